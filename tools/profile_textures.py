"""GPU cost of texture-mapped materials: a 480 x 640 pinhole frame in which every pixel hits a 2-triangle quad (tilted, UVs
0 .. 4 with wrap "repeat", so neighbouring pixels are about two texels of a 1024 x 1024 map apart and the sampler blends
two mip levels).  hit_attributes without maps, with a 1024^2 albedo map, and with 1024^2 albedo + roughness + normal maps:
per configuration the median of --iters synchronised calls (host clock around a device synchronise, as
tools/profile_objects.py) and the mean of a window of --window back-to-back calls between two device events; the bilinear
taps the sampler made (counted from the levels of detail it reports: 4 per level read), taps / s and the bytes gathered
(16 per tap) over the time, as a share of the HBM copy rate measured in the same run (a 1 GiB device-to-device copy, read
+ written bytes).  Then insert_object end to end on a seeded PanoMipNeRF: the untextured 1280-face icosphere of
profiles/objects_insert.txt, the quad without maps and the quad with the three maps.  One JSON line.

    python tools/profile_textures.py
    python tools/profile_textures.py --kernels     # no model: for rocprofv3 --kernel-trace --stats -d OUT -- python ...
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pano_nerf_amd import objects, views  # noqa: E402
from tools.profile_objects import icosphere, setup, timed  # noqa: E402


def windowed(fn, n):
    """mean ms per call of n back-to-back calls between two device events (after a warm-up call)"""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def quad(c2w, dev, size, maps):
    eye, right, up, fwd = c2w[:3, 3], c2w[:3, 0], c2w[:3, 1], -c2w[:3, 2]
    c = eye + 0.5 * fwd
    v = np.stack([c - 0.8 * right - 0.8 * up - 0.15 * fwd, c + 0.8 * right - 0.8 * up - 0.15 * fwd,
                  c + 0.8 * right + 0.8 * up + 0.15 * fwd, c - 0.8 * right + 0.8 * up + 0.15 * fwd]).astype(np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    kw = {}
    if maps:
        rng = np.random.default_rng(0)
        uv = np.array([[0, 0], [4, 0], [4, 4], [0, 4]], np.float32)
        kw = dict(uv=uv, albedo_map=objects.Texture(rng.integers(0, 256, (size, size, 3), dtype=np.uint8), srgb=True, device=dev))
        if maps == 3:
            nm = np.concatenate([0.5 + 0.2 * (rng.random((size, size, 2)) - 0.5), np.ones((size, size, 1))], 2)
            kw.update(roughness_map=objects.Texture((0.2 + 0.6 * rng.random((size, size))).astype(np.float32), device=dev),
                      normal_map=objects.Texture(nm.astype(np.float32), device=dev))
    return objects.VirtualObject(v, f, roughness=0.4, device=dev, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--kernels", action="store_true", help="hit_attributes only (no model, no insert_object)")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    c2w = views.look_at((0.1, 0.05, 0.2), (0.0, -0.1, -0.9))
    cam = views.perspective_camera(480, 640, fov_x_deg=60.0)
    R = cam.h * cam.w
    out = dict(frame="pinhole 480x640", rows=R, texture=f"{a.size}x{a.size}", iters=a.iters, window=a.window)
    # the HBM copy rate of this run
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    ms = windowed(lambda: dst.copy_(src), 20)
    copy_rate = 2 * src.numel() * 4 / (1e-3 * ms)
    out["hbm_copy_GBps"] = copy_rate / 1e9
    del src, dst
    o, d, radii = objects._frame_rays(cam, c2w, 0.0, 10.0, dev)
    objs = {"no_maps": quad(c2w, dev, a.size, 0), "albedo": quad(c2w, dev, a.size, 1), "three_maps": quad(c2w, dev, a.size, 3)}
    t, face, bary = objects.trace_mesh(o, d, objs["no_maps"].vertices, objs["no_maps"].faces)
    out["hit_pixels"] = int((face >= 0).sum())
    out["trace_ms"], _ = timed(lambda: objects.trace_mesh(o, d, objs["no_maps"].vertices, objs["no_maps"].faces), a.iters)
    for name, obj in objs.items():
        fn = lambda: objects.hit_attributes(obj, o, d, t, face, bary, radii=radii)
        out[f"hits_{name}_ms"], at = timed(fn, a.iters)
        out[f"hits_{name}_window_ms"] = windowed(fn, a.window)
        if obj.textured:
            s = objects.sample_textures(obj, at["mask"], face, bary, d, t, at["normals"], radii)
            lod = s["lod"][at["mask"]]
            n_maps = 1 if name == "albedo" else 3
            lv = lod[:, :n_maps] if n_maps == 3 else lod[:, :1]
            taps = int((4 * (1 + (lv != lv.floor()).to(torch.int64))).sum())
            extra = out[f"hits_{name}_window_ms"] - out["hits_no_maps_window_ms"]
            out[f"{name}_lod_min_mean_max"] = [float(lv.min()), float(lv.mean()), float(lv.max())]
            out[f"{name}_taps"] = taps
            out[f"{name}_sampler_window_ms"] = extra
            out[f"{name}_taps_per_s"] = taps / (1e-3 * extra)
            out[f"{name}_gathered_GBps"] = 16 * taps / (1e-3 * extra) / 1e9
            out[f"{name}_gathered_share_of_copy_rate"] = 16 * taps / (1e-3 * extra) / copy_rate
    if not a.kernels:
        model = setup()
        v, f = icosphere(3, 0.3, (0.0, -0.1, -0.9))
        sphere = objects.VirtualObject(v, f, roughness=0.4, device=dev)
        # alternate the three, twice, and keep both rounds: the spread between rounds is the noise of the comparison
        for rnd in (0, 1):
            for name, obj in (("icosphere_1280_untextured", sphere), ("quad_no_maps", objs["no_maps"]),
                              ("quad_three_maps", objs["three_maps"])):
                ms, _ = timed(lambda: objects.insert_object(model, cam, c2w, obj), a.iters)
                out.setdefault(f"insert_object_{name}_ms", []).append(ms)
        res = objects.insert_object(model, cam, c2w, objs["three_maps"])
        out["insert_object_quad_mask_pixels"] = int(res["mask"].sum())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
