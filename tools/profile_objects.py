"""GPU cost of virtual object insertion on a seeded PanoMipNeRF (default mlp_mode, default 128 samples per level): an
icosphere of 1280 or 81 920 faces inserted into a 480 x 640 pinhole frame and a 512 x 1024 panorama.  Per stage the
median of --iters synchronised runs after a warm-up call, one process: the probes (32 x 64 and 8 x 16), the tracer, shade
(Lambert and microfacet) on the frame's hit pixels, the 8 x 16 shadow over the frame, hit attributes + composite, next to
render_view of the same frame (rgb, depth, normal) measured in the same run, and insert_object end to end.  Also rays x
triangles / s of the tracer and BRDF evaluations / s of shade.  One JSON line per (mesh, frame).

--accel bvh (or both) adds the BVH path: MeshBVH.build as a whole and per stage, trace_mesh and shadow_ratio over a built
tree, build + trace + shadow as one call next to brute-force trace + shadow as one call (median and spread = max - min
of the repeats), insert_object(accel="bvh") with the build included, and the number of rays on which the two tracers
differ.  Level 8 is 1 310 720 faces.

    python tools/profile_objects.py                       # both meshes, both frames
    python tools/profile_objects.py --accel both --levels 3,6,8
    python tools/profile_objects.py --kernels              # the kernels alone, for a trace:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/profile_objects.py --kernels --iters 2 --levels 6 --frames pano
    PN_LIB=<another build of the library> python tools/profile_objects.py --kernels --accel bvh     # as tools/profile_conventions.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pano_nerf_amd as pn  # noqa: E402
from oracle import pano_oracle as orc  # noqa: E402
from pano_nerf_amd import _lib, lighting, objects, views  # noqa: E402

if os.environ.get("PN_LIB"):  # another build of the library, as tools/profile_conventions.py
    _lib.LIB_PATH = os.path.abspath(os.environ["PN_LIB"])


def setup():
    model = pn.PanoMipNeRF(rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    model.mlp.load_state_dict(orc.init_params(4, 5))
    return model.cuda()


def icosphere(level, radius, centre):
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1),
         (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius + np.asarray(centre)).astype(np.float32), np.array(f, dtype=np.int32)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), out


def timed_spread(fn, iters):
    """(median ms, max - min of the repeats in ms) of fn, as timed."""
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * (max(t) - min(t))


def bvh_stages(v, f, iters):
    """MeshBVH.build stage by stage (the same calls, each synchronised): ms per stage."""
    dev = v.device
    F, st = int(f.shape[0]), torch.cuda.current_stream(v.device).cuda_stream
    out = {}
    out["bvh_tri_setup_sphere_ms"], _ = timed(lambda: objects._prepare(v, f, dev, None), iters)
    tbox = torch.empty(F, 2, 4, device=dev)
    out["bvh_boxes_ms"], _ = timed(lambda: _lib.call("pn_bvh_boxes", F, int(v.shape[0]), v.data_ptr(), f.data_ptr(),
                                                     tbox.data_ptr(), st), iters)
    out["bvh_scene_box_ms"], scene = timed(lambda: torch.cat([tbox[:, 0, :3].amin(0), tbox[:, 1, :3].amax(0)]).contiguous(), iters)
    keys = torch.empty(F, dtype=torch.int64, device=dev)
    out["bvh_keys_ms"], _ = timed(lambda: _lib.call("pn_bvh_keys", F, tbox.data_ptr(), scene.data_ptr(), keys.data_ptr(), st), iters)
    out["bvh_sort_ms"], (skeys, order) = timed(lambda: torch.sort(keys, stable=True), iters)
    nodes = torch.empty(F - 1, 16, device=dev)
    parent, counters = (torch.empty(F, dtype=torch.int32, device=dev) for _ in range(2))
    out["bvh_tree_refit_ms"], _ = timed(lambda: _lib.call("pn_bvh_tree", F, skeys.data_ptr(), order.data_ptr(), tbox.data_ptr(),
                                                          nodes.data_ptr(), parent.data_ptr(), counters.data_ptr(), st), iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--kernels", action="store_true", help="the object kernels only (no scene render, no probes from the model)")
    ap.add_argument("--levels", default="3,6", help="icosphere subdivision levels (3: 1280 faces, 6: 81 920, 8: 1 310 720)")
    ap.add_argument("--accel", default="none", choices=("none", "bvh", "both"),
                    help="none: the brute-force tracer (the default path); bvh: the BVH path; both: both, side by side")
    ap.add_argument("--frames", default="both", choices=("both", "pinhole", "pano"), help="which of the two frames to run")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    eye, centre = (0.1, 0.05, 0.2), (0.0, -0.1, -0.9)
    c2w = views.look_at(eye, centre)
    frames = {"pinhole 480x640": views.perspective_camera(480, 640, fov_x_deg=60.0), "pano 512x1024": views.pano_camera(512, 1024)}
    frames = {k: c for k, c in frames.items() if a.frames == "both" or k.startswith(a.frames)}
    model = None if a.kernels else setup()
    g = torch.Generator(device="cuda").manual_seed(0)
    for level in (int(s) for s in a.levels.split(",")):
        v, f = icosphere(level, 0.3, centre)
        obj = objects.VirtualObject(v, f, roughness=None, device=dev)
        rough = objects.VirtualObject(v, f, roughness=0.4, device=dev)
        F = int(f.shape[0])
        for name, cam in frames.items():
            R = cam.h * cam.w
            out = dict(mesh_faces=F, frame=name, iters=a.iters)
            if model is not None:
                out["render_view_ms"], scene = timed(lambda: views.render_view(model, cam, c2w), a.iters)
                out["probes_32x64_ms"], probes = timed(lambda: lighting.light_probes(model, obj.centroid(), 32, 64), a.iters)
                out["probes_8x16_ms"], sprobe = timed(lambda: lighting.light_probes(model, obj.centroid(), 8, 16), a.iters)
                rows = lambda x: x.permute(0, 2, 3, 1).reshape(R, -1)
                s_dep, s_nor = rows(scene["fine_dep"]).reshape(R), rows(scene["fine_nor"])
            else:
                probes = torch.rand(1, 32, 64, 3, device=dev, generator=g).permute(0, 3, 1, 2) * 2.0
                sprobe = torch.rand(1, 8, 16, 3, device=dev, generator=g).permute(0, 3, 1, 2) * 2.0
                s_dep = torch.full((R,), 2.5, device=dev)
                s_nor = torch.nn.functional.normalize(torch.randn(R, 3, device=dev, generator=g), dim=1)
            o, d, _ = objects._frame_rays(cam, c2w, 0.0, 10.0, dev)
            brute, fast = a.accel in ("none", "both"), a.accel in ("bvh", "both")
            out["accel"] = a.accel
            if fast:
                out["bvh_build_ms"], out["bvh_build_spread_ms"] = timed_spread(
                    lambda: objects.MeshBVH.build(obj.vertices, obj.faces), a.iters)
                tree = objects.MeshBVH.build(obj.vertices, obj.faces)
                out.update(bvh_stages(obj.vertices, obj.faces, a.iters))
                out["bvh_trace_ms"], (t, face, bary) = timed(lambda: objects.trace_mesh(o, d, obj.vertices, obj.faces, accel=tree), a.iters)
            if brute:
                out["trace_ms"], (t, face, bary) = timed(lambda: objects.trace_mesh(o, d, obj.vertices, obj.faces), a.iters)
                out["trace_ray_triangles_per_s"] = R * F / (1e-3 * out["trace_ms"])
            if brute and fast:
                t2, face2, bary2 = objects.trace_mesh(o, d, obj.vertices, obj.faces, accel=tree)
                out["rays_bvh_differs_from_brute"] = int(((t2.view(torch.int32) != t.view(torch.int32)) | (face2 != face) |
                                                          (bary2.view(torch.int32) != bary.view(torch.int32)).any(1)).sum())
            out["hits_ms"], at = timed(lambda: objects.hit_attributes(obj, o, d, t, face, bary, s_dep), a.iters)
            m = at["mask"]
            n_hit = int(m.sum())
            out["hit_pixels"] = n_hit
            al, nr, vd = at["albedo"][m], at["normals"][m], at["viewdirs"][m]
            out["shade_lambert_ms"], _ = timed(lambda: objects.shade(probes, al, nr, vd), a.iters)
            out["shade_microfacet_ms"], _ = timed(lambda: objects.shade(probes, al, nr, vd, 0.4), a.iters)
            out["shade_microfacet_brdf_evals_per_s"] = n_hit * 32 * 64 / (1e-3 * out["shade_microfacet_ms"])
            sp = at["scene_points"]
            if fast:
                out["bvh_shadow_8x16_ms"], shadow = timed(
                    lambda: objects.shadow_ratio(sp, s_nor, sprobe, obj.vertices, obj.faces, accel=tree), a.iters)

                def through_bvh():
                    fresh = objects.MeshBVH.build(obj.vertices, obj.faces)
                    objects.trace_mesh(o, d, obj.vertices, obj.faces, accel=fresh)
                    return objects.shadow_ratio(sp, s_nor, sprobe, obj.vertices, obj.faces, accel=fresh)

                out["bvh_build_trace_shadow_ms"], out["bvh_build_trace_shadow_spread_ms"] = timed_spread(through_bvh, a.iters)
            if brute:
                out["shadow_8x16_ms"], shadow_b = timed(
                    lambda: objects.shadow_ratio(sp, s_nor, sprobe, obj.vertices, obj.faces), a.iters)

                def through_brute():
                    objects.trace_mesh(o, d, obj.vertices, obj.faces)
                    return objects.shadow_ratio(sp, s_nor, sprobe, obj.vertices, obj.faces)

                out["brute_trace_shadow_ms"], out["brute_trace_shadow_spread_ms"] = timed_spread(through_brute, a.iters)
                if fast:
                    out["shadow_bits_equal"] = bool(torch.equal(shadow.view(torch.int32), shadow_b.view(torch.int32)))
                shadow = shadow_b
            out["shadow_min"] = float(shadow.min())
            rgb, dep, orgb = (torch.empty(R, k, device=dev) for k in (3, 1, 3))
            m8, srgb = m.to(torch.uint8), torch.rand(R, 3, device=dev, generator=g)
            st = torch.cuda.current_stream(dev).cuda_stream
            out["composite_ms"], _ = timed(lambda: _lib.call(
                "pn_object_composite", R, m8.data_ptr(), orgb.data_ptr(), t.data_ptr(), srgb.data_ptr(), s_dep.data_ptr(),
                shadow.data_ptr(), rgb.data_ptr(), dep.data_ptr(), st), a.iters)
            if model is not None and brute:
                out["insert_object_lambert_ms"], _ = timed(lambda: objects.insert_object(model, cam, c2w, obj), a.iters)
                out["insert_object_microfacet_ms"], _ = timed(lambda: objects.insert_object(model, cam, c2w, rough), a.iters)
                stages = sum(out[k] for k in ("probes_32x64_ms", "probes_8x16_ms", "trace_ms", "hits_ms", "shade_microfacet_ms",
                                              "shadow_8x16_ms", "composite_ms"))
                out["object_stages_ms"] = stages
                out["object_stages_over_render_view"] = stages / out["render_view_ms"]
            if model is not None and fast:
                def with_build():  # a fresh object per call: the build is inside
                    return objects.insert_object(model, cam, c2w, objects.VirtualObject(obj.vertices, obj.faces), accel="bvh")

                out["insert_object_lambert_bvh_ms"], _ = timed(with_build, a.iters)
                out["insert_object_lambert_bvh_cached_ms"], _ = timed(lambda: objects.insert_object(model, cam, c2w, obj, accel="bvh"),
                                                                      a.iters)
                stages = sum(out[k] for k in ("probes_32x64_ms", "probes_8x16_ms", "bvh_build_ms", "bvh_trace_ms", "hits_ms",
                                              "shade_microfacet_ms", "bvh_shadow_8x16_ms", "composite_ms"))
                out["object_stages_bvh_ms"] = stages
                out["object_stages_bvh_over_render_view"] = stages / out["render_view_ms"]
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
