"""GPU cost of the sparse radiance volume (pano_nerf_amd.volume.SparseRadianceVolume) next to the dense one, in ONE process
on one device; writes the report profiles/volume_sparse.txt (and prints the same numbers as one JSON line).

1. bake_volume at --res^3 (sh_degree 1, albedo + normal): dense and sparse=True, once each after a small warm-up bake, with
   the peak of torch.cuda.max_memory_allocated over each call; at the default sigma_min (the untrained field is a fog:
   everything survives) and at a sigma_min that keeps about 5 % of the vertices (the 0.95 quantile of a 64^3 density grid).
2. Three occupancy levels of the default bake: "fog" (as baked), "ball" (tools/profile_volume.py's: emptied outside a ball
   in front of the pinhole camera) and "shell" (emptied outside a thin spherical shell around the camera: a surface).
   For each: bytes dense / sparse fp32 / sparse fp16, to_sparse and to_dense (whole calls, host clock, median of 3),
   pn_volume_pack alone (device events), and render_volume of a 480 x 640 pinhole frame and a 512 x 1024 panorama with
   skip on, dense against both sparse forms, alternating inside the same window loop; the taps and the bytes they gather
   (8 corners x element size per sigma tap, 8 x 3 K x element size more per sample with sigma > 0; a sparse sample reads
   one 4-byte table entry besides).  The run also checks that the three frames are equal where the contract says so.

    python tools/profile_sparse_volume.py [--res 256] [--window 5] [--out profiles/volume_sparse.txt]

The resource report of the kernels comes from the compiler, not from a run:
    PN_EXTRA=-Rpass-analysis=kernel-resource-usage bash pano-nerf_amd/csrc/build.sh 2>&1 | grep -A9 k_volume
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pano_nerf_amd import geometry, views, volume  # noqa: E402
from tools.profile_fusion import setup  # noqa: E402
from tools.profile_geometry import timed  # noqa: E402
from tools.profile_textures import windowed  # noqa: E402
from tools.profile_volume import copy_rate  # noqa: E402


def once(fn):
    """(seconds, peak bytes allocated during the call, result) of one synchronised call"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base, out


def masked(vol, keep):
    data = (vol.data.view(-1, vol.channels) * keep[:, None]).view(vol.data.shape).contiguous()
    return volume.RadianceVolume(data, vol.bounds, vol.sh_degree, vol._attrs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--far", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join("profiles", "volume_sparse.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_sparse_volume.py measures on a HIP device; none is visible")
    model, bounds, _ = setup()
    lo, hi = (np.asarray(c) for c in bounds)
    ext = hi - lo
    res = a.res
    out = dict(bounds=bounds, res=res, window=a.window, far=a.far, mlp_mode=model.mlp_mode)
    out["hbm_copy_TB_s"] = copy_rate()

    # ---- 1. the bake, dense and sparse
    volume.bake_volume(model, bounds, 32)
    volume.bake_volume(model, bounds, 32, sparse=True)
    pruned_min = float(torch.quantile(geometry.density_grid(model, bounds, 64).view(-1).float(), 0.95))
    vol = None
    for tag, kw in (("default", {}), ("pruned", dict(sigma_min=pruned_min))):
        sec_d, peak_d, dense = once(lambda: volume.bake_volume(model, bounds, res, **kw))
        kept = float((dense.sigma > 0).float().mean())
        if tag == "default":
            vol = dense
        else:
            del dense
        sec_s, peak_s, sp = once(lambda: volume.bake_volume(model, bounds, res, sparse=True, **kw))
        sec_h, peak_h, sp16 = once(lambda: volume.bake_volume(model, bounds, res, sparse=True, dtype=torch.float16, **kw))
        out[f"bake_{tag}"] = dict(sigma_min=kw.get("sigma_min"), kept_vertices=kept, present_bricks=sp.bricks / sp.table.numel(),
                                  dense_s=sec_d, dense_peak_MB=peak_d / 1e6, sparse_s=sec_s, sparse_peak_MB=peak_s / 1e6,
                                  sparse16_s=sec_h, sparse16_peak_MB=peak_h / 1e6, dense_MB=sp.dense_nbytes / 1e6,
                                  sparse_MB=sp.nbytes / 1e6, sparse16_MB=sp16.nbytes / 1e6)
        del sp, sp16
        torch.cuda.empty_cache()

    # ---- 2. three occupancy levels of the default bake
    pose = np.eye(4)
    pose[:3, 3] = 0.5 * (lo + hi)
    mean = geometry.grid_points(bounds, vol.resolution, 0.0, "cuda")[0]
    eye = torch.tensor(pose[:3, 3], device="cuda", dtype=torch.float32)
    centre = eye + torch.tensor([0.0, 0.0, -0.3 * ext[2]], device="cuda", dtype=torch.float32)
    ball = ((mean - centre) ** 2).sum(1) < (0.15 * float(ext.min())) ** 2
    dist = ((mean - eye) ** 2).sum(1).sqrt()
    shell = (dist - 0.35 * float(ext.min())).abs() < 1.5 * max(vol.step)
    del mean, dist
    cams = {"pinhole_480x640": views.perspective_camera(480, 640, fov_x_deg=70.0), "pano_512x1024": views.pano_camera(512, 1024)}
    K = (vol.sh_degree + 1) ** 2
    for level, keep in (("fog", None), ("ball", ball), ("shell", shell)):
        dense = vol if keep is None else masked(vol, keep)
        rec = dict(kept_vertices=float((dense.sigma > 0).float().mean()))
        rec["to_sparse_fp32_s"], sp = timed(lambda: dense.to_sparse(), 3)
        rec["to_sparse_fp16_s"], sp16 = timed(lambda: dense.to_sparse(torch.float16), 3)
        rec["to_dense_fp32_s"], _ = timed(lambda: sp.to_dense(), 3)
        rec["to_dense_fp16_s"], _ = timed(lambda: sp16.to_dense(), 3)
        for tag, s in (("fp32", sp), ("fp16", sp16)):
            rec[f"pack_{tag}_ms"] = windowed(lambda: volume._pack(s.resolution, s.channels, s.table, s.bricks, s.dtype,
                                                                  s.device, data=dense.data), a.window)
        rec.update(present_bricks=sp.bricks / sp.table.numel(), bricks=sp.bricks, dense_MB=sp.dense_nbytes / 1e6,
                   sparse_fp32_MB=sp.nbytes / 1e6, sparse_fp16_MB=sp16.nbytes / 1e6)
        forms = (("dense", dense, 4), ("fp32", sp, 4), ("fp16", sp16, 2))
        for cam_tag, cam in cams.items():
            rays = views.generate_camera_rays(cam, pose, 0.0, a.far, "cuda")
            render = lambda v: volume.render_volume(v, cam, pose, ("rgb", "depth"), 0.0, a.far, skip=True)
            frames = {tag: render(v) for tag, v, _ in forms}  # also the warm-up of every instance
            rec[f"{cam_tag}_fp32_equals_dense"] = all(torch.equal(frames["fp32"][k], frames["dense"][k]) for k in ("rgb", "depth"))
            f16 = render(sp16.to_dense())
            rec[f"{cam_tag}_fp16_equals_its_expansion"] = all(torch.equal(frames["fp16"][k], f16[k]) for k in ("rgb", "depth"))
            rec[f"{cam_tag}_fp16_max_abs_rgb_error"] = float((frames["fp16"]["rgb"] - frames["dense"]["rgb"]).abs().max())
            del frames, f16
            ms = {tag: [] for tag, _, _ in forms}
            for _ in range(3):  # alternate the three forms: three windows each, the median is reported
                for tag, v, _ in forms:
                    ms[tag].append(windowed(lambda: render(v), a.window))
            for tag, v, size in forms:
                taps = volume.march_rays(v, rays.origins, rays.directions, rays.near, rays.far, skip=True,
                                         outputs=("taps",))["taps"].sum(0).tolist()
                gathered = 8.0 * size * (taps[0] + 3 * K * taps[1])
                med = float(np.median(ms[tag]))
                rec[f"{cam_tag}_{tag}"] = dict(ms=med, ms_min=min(ms[tag]), ms_max=max(ms[tag]), sigma_taps=taps[0],
                                               colour_taps=taps[1], gathered_GB=gathered / 1e9,
                                               gathered_TB_s=gathered / (1e-3 * med) / 1e12)
        out[level] = rec
        del sp, sp16, dense
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(report(out))


def report(o):
    """the numbers of one run as the text of profiles/volume_sparse.txt"""
    res = o["res"]
    L = [f"The sparse radiance volume on one MI355X, tools/profile_sparse_volume.py --res {res} --window {o['window']}: one process, "
         "one run, run once.",
         f"Seeded PanoMipNeRF (mlp_mode {o['mlp_mode']!r}), tools/profile_fusion.py's box, camera in the middle, near 0, far {o['far']:g},",
         "sh_degree 1 + albedo + normal (19 channels).  Render times are device-event windows of render_volume(rgb, depth), skip on,",
         "everything the call does included; the three forms alternate, three windows each: median (min - max).",
         f"HBM copy rate of this run: {o['hbm_copy_TB_s']:.2f} TB/s.", ""]
    L.append(f"1. bake_volume at {res}^3, once each (host clock; peak = torch.cuda.max_memory_allocated over the call, above what "
             "was allocated before it)")
    for tag in ("default", "pruned"):
        b = o[f"bake_{tag}"]
        L.append(f"   {tag} sigma_min{'' if b['sigma_min'] is None else ' = %.4g' % b['sigma_min']}: {100 * b['kept_vertices']:.1f} % of the "
                 f"vertices kept, {100 * b['present_bricks']:.1f} % of the bricks present")
        L.append(f"     dense        {b['dense_s']:.3f} s   peak {b['dense_peak_MB']:.0f} MB   result {b['dense_MB']:.0f} MB")
        L.append(f"     sparse fp32  {b['sparse_s']:.3f} s   peak {b['sparse_peak_MB']:.0f} MB   result {b['sparse_MB']:.0f} MB")
        L.append(f"     sparse fp16  {b['sparse16_s']:.3f} s   peak {b['sparse16_peak_MB']:.0f} MB   result {b['sparse16_MB']:.0f} MB")
    L.append("")
    L.append("2. three occupancy levels of the default bake")
    for level in ("fog", "ball", "shell"):
        r = o[level]
        L.append(f"   {level}: {100 * r['kept_vertices']:.2f} % of the vertices positive, {r['bricks']} bricks = "
                 f"{100 * r['present_bricks']:.2f} % present")
        L.append(f"     bytes      dense {r['dense_MB']:.1f} MB   sparse fp32 {r['sparse_fp32_MB']:.1f} MB   sparse fp16 "
                 f"{r['sparse_fp16_MB']:.1f} MB")
        L.append(f"     to_sparse  fp32 {1e3 * r['to_sparse_fp32_s']:.2f} ms   fp16 {1e3 * r['to_sparse_fp16_s']:.2f} ms (whole call: "
                 "occupancy, prefix sum, pack, table check, a host sync for B, one for the check, one more for the fp16 overflow "
                 f"test);   pn_volume_pack alone fp32 {r['pack_fp32_ms']:.3f} ms   "
                 f"fp16 {r['pack_fp16_ms']:.3f} ms")
        L.append(f"     to_dense   fp32 {1e3 * r['to_dense_fp32_s']:.2f} ms   fp16 {1e3 * r['to_dense_fp16_s']:.2f} ms")
        for cam in ("pinhole_480x640", "pano_512x1024"):
            L.append(f"     {cam}: fp32 frame equals dense: {r[cam + '_fp32_equals_dense']};  fp16 frame equals its expansion's: "
                     f"{r[cam + '_fp16_equals_its_expansion']};  max |rgb fp16 - rgb dense| {r[cam + '_fp16_max_abs_rgb_error']:.3g}")
            for tag in ("dense", "fp32", "fp16"):
                c = r[f"{cam}_{tag}"]
                L.append(f"       {tag:5s}  {c['ms']:.3f} ms ({c['ms_min']:.3f} - {c['ms_max']:.3f})   "
                         f"x dense {c['ms'] / r[cam + '_dense']['ms']:.2f}   sigma taps {c['sigma_taps'] / 1e6:.1f} M   colour taps "
                         f"{c['colour_taps'] / 1e6:.1f} M   gathered {c['gathered_GB']:.2f} GB = {c['gathered_TB_s']:.2f} TB/s")
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    main()
