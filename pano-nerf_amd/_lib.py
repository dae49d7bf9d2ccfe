"""ctypes binding of libpanonerf_hip.so (the C ABI declared in include/panonerf_hip.h).

The product path has NO fallback: if the shared library is missing or a symbol is absent this
module raises at import of the first entry point, and every non-zero status is raised as
RuntimeError.  Build with ``python __graft_entry__.py`` or ``pano-nerf_amd/csrc/build.sh``.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpanonerf_hip.so")

_P, _I, _L, _F, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
_CODES = {"p": _P, "i": _I, "l": _L, "f": _F, "d": _D}

# name -> (restype code, argument codes); order = include/panonerf_hip.h
SIGNATURES = {
    "pn_strerror": ("s", "i"),
    "pn_abi_version": ("i", ""),
    "pn_pad_rows": ("l", "l"),
    "pn_param_layout": ("l", "ip"),
    "pn_wpack_floats": ("l", "i"),
    "pn_pack_weights": ("i", "pipp"),
    "pn_raygen_pano": ("i", "iipff" + "p" * 8 + "p"),
    "pn_lit_rays": ("i", "idddpp"),
    "pn_gather_rays": ("i", "llpppp"),
    "pn_sample_pano_rays": ("i", "liiippffp" + "p" * 9 + "p"),
    "pn_sample_coarse": ("i", "lii" + "p" * 9 + "p"),
    "pn_resample": ("i", "lippfp" + "p" * 6 + "p"),
    "pn_sample_env": ("i", "lii" + "p" * 11 + "p"),
    "pn_ipe_encode": ("i", "lpppp"),
    "pn_pos_enc_view": ("i", "lppp"),
    "pn_mlp_forward": ("i", "lili" + "p" * 12 + "p"),
    "pn_density_grad": ("i", "lif" + "p" * 10 + "p"),
    "pn_mlp_backward_work_floats": ("l", "lill"),
    "pn_mlp_backward": ("i", "lilif" + "p" * 16 + "lii" + "p" * 6 + "pp"),
    "pn_composite_forward": ("i", "liiffi" + "pppp" + "l" + "pppp" + "p"),
    "pn_composite_backward": ("i", "liiffi" + "pppp" + "l" + "ppppp" + "p"),
    "pn_surf_gather_forward": ("i", "lii" + "p" * 7 + "p"),
    "pn_surf_gather_backward": ("i", "lii" + "p" * 10 + "p"),
    "pn_surface_forward": ("i", "li" + "p" * 7 + "p"),
    "pn_surface_backward": ("i", "li" + "p" * 10 + "p"),
    "pn_env_origin_backward": ("i", "lipppp"),
    "pn_tonemap_loss": ("i", "l" + "p" * 6 + "fff" + "p" * 6 + "p"),
    "pn_adam_step": ("i", "lppppffffifp"),
    "pn_adam_step_dev": ("i", "lpppppfffpfp"),
    "pn_gemm_nt": ("i", "liipipipippiip"),
    "pn_gemm_tn_work_floats": ("l", "lii"),
    "pn_gemm_tn": ("i", "liipipipiipp"),
    "pn_chain_tile": ("i", ""),
    "pn_chain_pack_bytes": ("l", "i"),
    "pn_chain_pack": ("i", "piipp"),
    "pn_chain_acts_floats": ("l", "l"),
    "pn_chain_amax_slots": ("i", ""),
    "pn_chain_forward": ("i", "lilii" + "p" * 11 + "iip"),
    "pn_chain_density_grad": ("i", "liif" + "p" * 7 + "ippiip"),
    "pn_chain_tangent": ("i", "lii" + "p" * 10 + "iip"),
    "pn_chain_backward": ("i", "liif" + "p" * 15 + "iip"),
    "pn_chain_wgrad_work_floats": ("l", ""),
    "pn_chain_q24_slots": ("i", "iii"),
    "pn_chain_wgrad": ("i", "ipiippliiip"),
    "pn_metrics_work_doubles": ("l", "iii"),
    "pn_metric_sums": ("i", "iii" + "plli" * 2 + "ppp"),
    "pn_metric_ssim": ("i", "iii" + "plli" * 2 + "ipd" + "pppp"),
    "pn_metric_normals": ("i", "ii" + "pll" * 2 + "i" + "ppp"),
    "pn_metric_depth": ("i", "l" + "pl" * 3 + "ppp"),
    "pn_grid_points": ("i", "iiill" + "f" * 7 + "ppp"),
    "pn_field_epilogue": ("i", "liff" + "p" * 7 + "p"),
    "pn_mt_work_bytes": ("l", "iii"),
    "pn_mt_count": ("i", "iiipfppp"),
    "pn_mt_emit": ("i", "iiipfpll" + "f" * 6 + "ppp"),
    "pn_probe_sh_work_doubles": ("l", "lii"),
    "pn_probe_sh": ("i", "liip" + "lll" + "pppp" + "p"),
    "pn_probe_irradiance": ("i", "liip" + "lll" + "pp" + "lpi" + "p" + "p"),
    "pn_sh_volume_irradiance": ("i", "iii" + "f" * 6 + "plppp" + "p"),
    "pn_prefilter_work_doubles": ("l", "liil"),
    "pn_prefilter": ("i", "liip" + "lll" + "pp" + "lpid" + "pp" + "p"),
    "pn_brdf_lut": ("i", "iipp"),
    "pn_ibl_shade": ("i", "lii" + "pipip" + "pppp" + "ff" + "ppp" + "p"),
    "pn_sample_pinhole_rays": ("i", "liiipppffp" + "p" * 9 + "p"),
    "pn_to_frame": ("i", "iiipllfffppp" + "p"),
    "pn_sample_camera_rays": ("i", "liiiipppffp" + "p" * 9 + "p"),
    "pn_reproject": ("i", "iiiiipiiippifplllppp"),
    "pn_warp_splat": ("i", "iiiipppiiiippifpp"),
    "pn_warp_resolve": ("i", "iiiiiiii" + "ppp" + "lllf" + "pppp" + "p"),
    "pn_warp_blend": ("i", "iiiii" + "ppp" + "ff" + "ppp" + "p"),
    "pn_fill_holes_work_floats": ("l", "iiiii"),
    "pn_fill_holes": ("i", "iiii" + "pppp" + "ifi" + "ppl" + "p"),
    "pn_ingest_image": ("i", "iiiipiiiiiiffpp"),
    "pn_tri_setup": ("i", "llpppp"),
    "pn_trace_mesh": ("i", "lpplpppi" + "pppp" + "p"),
    "pn_shade": ("i", "liiiplll" + "pppppp" + "fip" + "pppp" + "p"),
    "pn_shadow_ratio": ("i", "liipllppppflppp" + "p"),
    "pn_object_hits": ("i", "lpppppp" + "lplp" + "pp" + "fff" + "ip" + "p" * 7 + "p"),
    "pn_object_composite": ("i", "l" + "p" * 8 + "p"),
    "pn_bvh_boxes": ("i", "llpppp"),
    "pn_bvh_keys": ("i", "lpppp"),
    "pn_bvh_tree": ("i", "lpppppp" + "p"),
    "pn_trace_mesh_bvh": ("i", "lpplpppi" + "pppp" + "p"),
    "pn_shadow_ratio_bvh": ("i", "liipllppppflpppp" + "p"),
    "pn_tex_floats": ("l", "ii"),
    "pn_tex_ingest": ("i", "iiiipppp"),
    "pn_tex_pyramid": ("i", "iipp"),
    "pn_texture_hits": ("i", "l" + "p" * 7 + "lplp" + "lpp" + "pii" * 3 + "ii" + "pppp" + "p"),
    "pn_atlas_uv": ("i", "liipp"),
    "pn_atlas_texels": ("i", "iill" + "ppp" + "pppppp" + "p"),
    "pn_atlas_encode_normals": ("i", "iill" + "pp" + "ppppp" + "p"),
    "pn_atlas_quantize": ("i", "lippp" + "p"),
    "pn_relight": ("i", "l" + "pppppp" + "ip" + "iiip" + "fffff" + "i" + "ppp" + "p"),
    "pn_emitter_threshold": ("i", "liip" + "lll" + "pdp" + "p"),
    "pn_emitter_labels": ("i", "liip" + "lll" + "pppp" + "p"),
    "pn_emitter_compact": ("i", "liippp" + "p"),
    "pn_emitter_stats": ("i", "liip" + "lll" + "ppp" + "il" + "pp" + "p" * 10 + "p"),
    "pn_tsdf_integrate": ("i", "iii" + "f" * 6 + "iiii" + "ppppp" + "fff" + "pp" + "p"),
    "pn_mesh_check": ("i", "llppp" + "p"),
    "pn_mesh_components": ("i", "llpppp" + "p"),
    "pn_mesh_labels": ("i", "ll" + "p" * 6 + "p"),
    "pn_mesh_component_stats": ("i", "lll" + "ppppp" + "lp" + "pppppp" + "p"),
    "pn_cluster_keys": ("i", "lp" + "ffff" + "lll" + "p" + "p"),
    "pn_cluster_faces": ("i", "lll" + "pppp" + "p"),
    "pn_cluster_solve": ("i", "lll" + "pppp" + "ffff" + "lll" + "ppppp" + "d" + "pppp" + "p"),
    "pn_closest_point": ("i", "lplplp" + "f" + "pppp" + "p"),
    "pn_closest_point_bvh": ("i", "lplplpp" + "f" + "pppp" + "p"),
    "pn_face_areas": ("i", "llppp" + "p"),
    "pn_face_weights": ("i", "lppp" + "p"),
    "pn_sample_surface": ("i", "llll" + "ppp" + "ppp" + "p"),
    "pn_winding": ("i", "lplplp" + "p" + "p"),
    "pn_bvh_moments": ("i", "llpp" + "ppp" + "p"),
    "pn_winding_bvh": ("i", "lplplp" + "pp" + "f" + "p" + "p"),
    "pn_volume_bricks": ("l", "iii"),
    "pn_volume_occupancy": ("i", "iiii" + "pp" + "p"),
    "pn_volume_march": ("i", "liiiii" + "pp" + "ffffff" + "pppp" + "ff" + "ppppp" + "p"),
    "pn_volume_march_bwd": ("i", "liiiii" + "pp" + "ffffff" + "pppp" + "ff" + "pp" + "d" + "pp" + "p"),
    "pn_volume_grad_finish": ("i", "liip" + "d" + "ppi" + "p"),
    "pn_volume_pack": ("i", "iiii" + "pl" + "pplp" + "ip" + "p"),
    "pn_volume_unpack": ("i", "iiii" + "pl" + "pi" + "p" + "p"),
    "pn_volume_march_sparse": ("i", "liiiii" + "pp" + "ii" + "ffffff" + "pppp" + "ff" + "ppppp" + "p"),
    "pn_mfma_probe": ("i", "piip"),
    "pn_prof_enable": ("i", "i"),
    "pn_prof_read": ("i", "ippp"),
}

_lib = None


def load():
    """Load the shared library (once) and attach the prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension is not built (run `python __graft_entry__.py` "
            "or pano-nerf_amd/csrc/build.sh).  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = ctypes.c_char_p if res == "s" else _CODES[res]
        fn.argtypes = [_CODES[c] for c in args]
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        msg = load().pn_strerror(int(code)).decode()
        raise RuntimeError(f"{what} failed: {msg} (code {code})")


def call(name, *args):
    """Call an int-returning entry point and raise on a non-zero status."""
    check(getattr(load(), name)(*args), name)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream(dev):
    """Raw handle of the device's current HIP stream: the last argument of every launching entry point."""
    return torch.cuda.current_stream(dev).cuda_stream
