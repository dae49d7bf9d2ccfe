"""GPU cost of the novel-view module on a seeded PanoMipNeRF (default mlp_mode, default 128 samples per level).

--what path: a 24-frame interpolate_path at --size, rendered with render_path for kinds ldr, depth, normal ("basic",
no light gather) and with every output ("all": ldr_surf and albedo added), and, in the same process and alternating,
render_image on the same rays frame by frame (the yardstick).  --repeats rounds of the three; frames/s, the median and
the spread (max - min) of each are printed as one JSON line.

--what kernels: the ray sampler of every camera kind (CameraRig.sample over every ray of the path; the pinhole at --size,
the others at the nearest shape of theirs) and pn_to_frame for each kind at --size, with their bytes moved.  Run it under
rocprofv3 for the kernel trace:

--what cameras: render_view of a 6 x 256 cube map and of a 512 x 1024 stereo-panorama pair next to the panorama
render_view of the same run (rays/s: the renderer is the same, so should the rate be), and views.reproject of a
512 x 1024 x 3 panorama to a 6 x 512 cube at samples 1 and 4 and of 64 probes of 32 x 64 to cubes of 16, each as device
time and as bytes moved (source read once + output and coverage written) over that time, next to the HBM copy rate.

    python tools/profile_views.py --what path --size 480x640
    python tools/profile_views.py --what cameras
    python tools/profile_views.py --what path --size 120x160
    python tools/profile_views.py --what kernels --size 480x640
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/profile_views.py --what kernels --size 480x640
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
from pano_nerf_amd import views  # noqa: E402
from pano_nerf_amd.rays import CameraRig  # noqa: E402

BASIC = ("ldr", "depth", "normal")
ALL = ("ldr", "ldr_surf", "depth", "normal", "albedo")


def setup():
    model = pn.PanoMipNeRF(rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    model.mlp.load_state_dict(orc.init_params(4, 5))
    return model.cuda()


def poses(frames):
    """interpolate_path through frames // 8 look-at poses around the origin (8 frames per leg)"""
    rng = np.random.default_rng(0)
    keys = np.stack([views.look_at(rng.uniform(-1.0, 1.0, 3) + np.array([0.0, 0.0, 2.5]), [0, 0, 0])
                     for _ in range(max(1, frames // 8))])
    return views.interpolate_path(keys, 24)[:frames]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def event_ms(fn, iters):
    """device time per call from HIP events around `iters` back-to-back calls (after a warm-up call)"""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


HBM_COPY_TB_S = 6.29  # measured float4 copy rate of one MI355X (8.0 TB/s spec)


def cameras(repeats):
    out = dict(what="cameras", hbm_copy_tb_per_s=HBM_COPY_TB_S, repeats=repeats)
    model = setup()
    c2w = views.look_at([0.2, 0.1, 0.3], [0.0, 0.0, -1.0])
    out.update(mlp_mode=model.mlp_mode, num_samples=model.num_samples)
    ipd = 0.064
    legs = {"render_view_pano_512x1024": (512 * 1024, lambda: views.render_view(model, views.pano_camera(512, 1024), c2w)),
            "render_view_cube_6x256": (6 * 256 * 256, lambda: views.render_view(model, views.cubemap_camera(256), c2w)),
            "render_stereo_pano_512x1024": (2 * 512 * 1024, lambda: views.render_stereo_pano(model, 512, 1024, ipd, c2w))}
    views.render_view(model, views.pano_camera(64, 128), c2w)  # warm-up: allocator, packed weights
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, (_, fn) in legs.items():
            times[k].append(timed(fn))
    for k, t in times.items():
        med = float(np.median(t))
        out[k] = dict(rays=legs[k][0], seconds=t, median_s=med, spread_s=float(max(t) - min(t)), rays_per_s=legs[k][0] / med)
    g = torch.Generator(device="cuda").manual_seed(0)
    pano = torch.rand(1, 3, 512, 1024, device="cuda", generator=g) * 4.0
    probes = (torch.rand(64, 32, 64, 3, device="cuda", generator=g) * 4.0).permute(0, 3, 1, 2)  # as light_probes returns them
    res = {}
    for name, x, src, dst, k in (("pano_512x1024x3_to_cube_512_s1", pano, views.pano_camera(512, 1024), views.cubemap_camera(512), 1),
                                 ("pano_512x1024x3_to_cube_512_s4", pano, views.pano_camera(512, 1024), views.cubemap_camera(512), 4),
                                 ("64_probes_32x64_to_cube_16_s4", probes, views.pano_camera(32, 64), views.cubemap_camera(16), 4)):
        ms = event_ms(lambda: views.reproject(x, src, dst, samples=k), 50)
        N, C = int(x.shape[0]), int(x.shape[1])
        byts = 4 * (N * C * src.h * src.w + N * C * dst.h * dst.w + dst.h * dst.w)
        res[name] = dict(call_ms=ms, bytes=byts, tb_per_s=byts / (ms * 1e-3) / 1e12,
                         share_of_hbm_copy=byts / (ms * 1e-3) / 1e12 / HBM_COPY_TB_S,
                         subsamples_per_s=N * dst.h * dst.w * k * k / (ms * 1e-3))
    out["reproject"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("path", "kernels", "cameras"), required=True)
    ap.add_argument("--size", default="480x640")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.what == "cameras":
        print(json.dumps(cameras(a.repeats)))
        return
    H, W = (int(s) for s in a.size.split("x"))
    cam = views.perspective_camera(H, W, fov_x_deg=60.0)
    path = poses(a.frames)
    n = path.shape[0]
    out = dict(what=a.what, size=[H, W], frames=n)
    if a.what == "path":
        model = setup()
        env = pn.generate_lit_rays(10, 0.01)
        out.update(mlp_mode=model.mlp_mode, num_samples=model.num_samples, repeats=a.repeats)

        def per_frame_render_image():
            for c2w in path:
                rays = views.generate_perspective_rays(cam, c2w)
                pn.render_image(model, pn.Rays(*[x.view(1, H, W, -1) for x in rays]), env, H, W)

        legs = {"render_path_basic": lambda: views.render_path(model, cam, path, env, kinds=BASIC),
                "render_path_all": lambda: views.render_path(model, cam, path, env, kinds=ALL),
                "render_image": per_frame_render_image}
        # warm-up (allocator, packed weights): one frame of each
        views.render_path(model, cam, path[:1], env, kinds=ALL)
        views.render_path(model, cam, path[:1], env, kinds=BASIC)
        rays = views.generate_perspective_rays(cam, path[0])
        pn.render_image(model, pn.Rays(*[x.view(1, H, W, -1) for x in rays]), env, H, W)
        times = {k: [] for k in legs}
        for _ in range(a.repeats):
            for k, fn in legs.items():
                times[k].append(timed(fn))
        for k, t in times.items():
            med = float(np.median(t))
            out[k] = dict(seconds=t, median_s=med, spread_s=float(max(t) - min(t)), frames_per_s=n / med,
                          ms_per_frame=1e3 * med / n)
        ri = out["render_image"]["median_s"]
        out["ratio_all_to_render_image"] = out["render_path_all"]["median_s"] / ri
        out["ratio_basic_to_render_image"] = out["render_path_basic"]["median_s"] / ri
    else:
        res = {}
        dev = torch.device("cuda", torch.cuda.current_device())
        S = max(2, round((H * W / 6) ** 0.5))
        for name, c in (("pinhole", cam), ("pano", views.pano_camera(H, W)), ("cube", views.cubemap_camera(S)),
                        ("fisheye", views.fisheye_camera(H, W)), ("stereo_pano", views.stereo_pano_camera(H, W, 0.064, "left"))):
            rig = CameraRig(c, path, dev)
            B = len(rig)
            idx = torch.arange(B, dtype=torch.int64, device=dev)
            ms = event_ms(lambda: rig.sample(idx, 0.0, 10.0), 5)
            byts = B * (8 + 15 * 4)  # index in, 15 floats of ray out
            res[f"sample_{name}_rays"] = dict(rays=B, call_ms=ms, bytes=byts, tb_per_s=byts / (ms * 1e-3) / 1e12)
        g = torch.Generator(device="cuda").manual_seed(0)
        img3 = (torch.rand(H * W, 3, device="cuda", generator=g) * 2.0).view(1, H, W, 3).permute(0, 3, 1, 2)
        dep = (torch.rand(H * W, 1, device="cuda", generator=g) * 8.0).view(1, H, W, 1).permute(0, 3, 1, 2)
        for kind, x, rd in (("ldr", img3, 12), ("normal", img3, 12), ("depth", dep, 8)):
            ms = event_ms(lambda: views.to_frame(x, kind, 0.0, 10.0), 20)
            byts = H * W * (rd + 3)  # depth reads its image twice (min / max, then the frame)
            res["pn_to_frame/" + kind] = dict(call_ms=ms, bytes=byts, tb_per_s=byts / (ms * 1e-3) / 1e12)
        out.update(kernels=res)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
