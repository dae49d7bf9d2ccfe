"""GPU cost of the radiance volume's gradient and of fit_volume (pano_nerf_amd.volume).  One process, one text report:

1. march_rays_grad next to march_rays on the same rays (device-event windows): 4096 and 65 536 random rays of a pinhole
   camera and its 480 x 640 frame in pixel order, at 256^3 and SH degree 0 / 1 / 2, on the fog (the seeded field as baked)
   and on the ball (the same volume emptied outside a ball), tools/profile_volume.py's two levels.  The upstream gradient
   is that of a mean squared error with errors of size 1: normal values times 2 / (3 R).  Contributions are counted from
   the forward's "taps": 8 (1 + 3 K) per compositing sample.  That is an upper bound of the atomics issued: a
   contribution that rounds to 0 quanta, or whose colour is clamped, issues none.
2. pn_volume_grad_finish (with and without clear) next to the HBM copy rate of this run.
3. fit_volume steps per second at 128^3 and 256^3 (degree 1, 4096 rays per step).
4. The sweep the two default learning rates come from, and the PSNR of render_volume against render_view on held-out
   poses before and after fitting, for tools/profile_fusion.py's model.

    python tools/profile_volume_fit.py [--res 256] [--fit-res 128] [--steps 200] [--window 3]

profiles/volume_fit.txt is this report as printed, followed by what does not come from a run of this tool: the loss ratios
the device tests print, and the compiler's registers and scratch per kernel instance,
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --save-temps -c pano-nerf_amd/csrc/pn_volume.hip
    grep -E '\\.(name|vgpr_count|private_segment_fixed_size):' pn_volume-hip-amdgcn-amd-amdhsa-gfx950.s
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pano_nerf_amd import geometry, views, volume  # noqa: E402
from tools.profile_fusion import setup  # noqa: E402
from tools.profile_textures import windowed  # noqa: E402
from tools.profile_volume import copy_rate  # noqa: E402

FLOAT_ATOMIC_TB_S = 1.3  # the guide's rate of contiguous float atomics, in added bytes


def say(line=""):
    print(line, flush=True)


def ball_of(vol, centre, radius):
    mean = geometry.grid_points(vol.bounds, vol.resolution, 0.0, "cuda")[0]
    keep = ((mean - torch.tensor(centre, device="cuda", dtype=torch.float32)) ** 2).sum(1) < radius ** 2
    return volume.RadianceVolume((vol.data.view(-1, vol.channels) * keep[:, None]).view(vol.data.shape).contiguous(),
                                 vol.bounds, vol.sh_degree, vol._attrs)


def psnr(a, b):
    return -10.0 * math.log10(float(((a - b) ** 2).mean()))


def held_out_psnr(vol, cam, poses, targets, far):
    got = torch.cat([volume.render_volume(vol, cam, p, ("rgb",), 0.0, far)["rgb"] for p in poses])
    return psnr(got, targets)


def poses_in(bounds, count, seed):
    rng = np.random.default_rng(seed)
    lo, hi = (np.asarray(c) for c in bounds)
    out = []
    for _ in range(count):
        eye = lo + (0.3 + 0.4 * rng.random(3)) * (hi - lo)
        out.append(views.look_at(eye, eye + rng.standard_normal(3)))
    return np.stack(out).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--fit-res", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--window", type=int, default=3)
    ap.add_argument("--far", type=float, default=10.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_volume_fit.py measures on a HIP device; none is visible")
    model, bounds, _ = setup()
    lo, hi = (np.asarray(c) for c in bounds)
    ext = hi - lo
    copy = copy_rate()
    say(f"The radiance volume's gradient on one MI355X, tools/profile_volume_fit.py --res {a.res} --fit-res {a.fit_res} "
        f"--steps {a.steps} --window {a.window}: one process, one run.")
    say(f"Seeded PanoMipNeRF (mlp_mode {model.mlp_mode!r}), tools/profile_fusion.py's box, near 0, far {a.far:g}, no attribute "
        f"channels.  Times are device-event windows of {a.window} calls after a warm-up call, everything the call does included.")
    say(f"HBM copy rate of this run: {copy:.2f} TB/s.  The guide's rate of contiguous float atomics: {FLOAT_ATOMIC_TB_S} TB/s of added bytes.")
    say()

    pose = np.eye(4)
    pose[:3, 3] = 0.5 * (lo + hi)
    centre = pose[:3, 3] + np.array([0.0, 0.0, -0.3 * ext[2]])
    cam = views.perspective_camera(480, 640, fov_x_deg=70.0)
    frame = views.generate_camera_rays(cam, pose, 0.0, a.far, "cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    sets = {}
    for count in (4096, 65536):
        idx = torch.randint(0, 480 * 640, (count,), device="cuda", generator=gen)
        sets[f"{count} random rays"] = tuple(x[idx].contiguous() for x in (frame.origins, frame.directions, frame.near, frame.far))
    sets["480 x 640 frame, pixel order"] = (frame.origins, frame.directions, frame.near, frame.far)

    say(f"1. march_rays_grad next to march_rays (rgb, acc) at {a.res}^3")
    finish = []
    for deg in (0, 1, 2):
        K = (deg + 1) ** 2
        fog = volume.bake_volume(model, bounds, a.res, deg, attributes=())
        levels = {"fog": fog, "ball": ball_of(fog, centre, 0.15 * float(ext.min()))}
        N = fog.data.numel() // fog.channels
        sums = torch.zeros(N, 1 + 3 * K, dtype=torch.int64, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        for level, vol in levels.items():
            say(f"   degree {deg}, {level}: {100 * float(vol.occupancy.float().mean()):.2f} % of the bricks occupied, "
                f"sums {sums.numel() * 8 / 1e6:.0f} MB")
            for tag, rows in sets.items():
                R = rows[0].shape[0]
                g = torch.randn(R, 3, device="cuda", generator=gen) * (2.0 / (3 * R))
                fwd = windowed(lambda: volume.march_rays(vol, *rows, outputs=("rgb", "acc")), a.window)
                bwd = windowed(lambda: volume.march_rays_grad(vol, *rows, g, None, sums=sums, flag=flag), a.window)
                taps = volume.march_rays(vol, *rows, outputs=("taps",))["taps"].sum(0).tolist()
                contrib = taps[1] * 8 * (1 + 3 * K)
                rate = contrib / (1e-3 * bwd)
                say(f"     {tag:29s} forward {fwd:8.3f} ms   backward {bwd:9.3f} ms   x forward {bwd / fwd:6.1f}   "
                    f"compositing samples {taps[1] / 1e6:7.2f} M   contributions <= {contrib / 1e9:7.3f} G = "
                    f"{rate / 1e9:6.1f} G/s = {8 * rate / 1e12:5.2f} TB/s of added bytes ({8 * rate / 1e12 / FLOAT_ATOMIC_TB_S:4.2f} x the float rate)")
            assert int(flag) == 0
            sums.zero_()
        if deg == 1:
            for clear in (False, True):
                ms = windowed(lambda: volume.finish_grad(fog, sums, flag, clear=clear), a.window)
                moved = sums.numel() * 8 * (2 if clear else 1) + fog.data.numel() * 4
                finish.append(f"     clear={clear!s:5s} {ms:7.3f} ms   {moved / 1e6:.0f} MB read and written = "
                              f"{moved / (1e-3 * ms) / 1e12:.2f} TB/s ({moved / (1e-3 * ms) / 1e12 / copy:.2f} x the copy rate; the "
                              "call allocates its output)")
        del fog, levels, sums
    say()
    say(f"2. pn_volume_grad_finish at {a.res}^3, degree 1")
    for line in finish:
        say(line)
    say()

    say("3. fit_volume, degree 1, 4096 rays per step, a 120 x 160 pinhole camera at 8 poses")
    small = views.perspective_camera(120, 160, fov_x_deg=70.0)
    train_poses, test_poses = poses_in(bounds, 8, 1), poses_in(bounds, 3, 2)
    render = lambda ps: torch.cat([views.render_view(model, small, p, outputs=("rgb",), far=a.far)["fine_rgb"] for p in ps])
    train, test = render(train_poses), render(test_poses)
    for res in (a.fit_res, a.res):
        vol = volume.bake_volume(model, bounds, res, 1, attributes=())
        volume.fit_volume(vol, train, small, train_poses, 5, far=a.far)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        volume.fit_volume(vol, train, small, train_poses, a.steps, far=a.far)
        torch.cuda.synchronize()
        say(f"   {res}^3: {a.steps / (time.perf_counter() - t0):7.1f} steps/s ({a.steps} steps, host clock around a synchronise)")
        del vol
    say()

    say(f"4. held-out PSNR of render_volume against render_view ({len(test_poses)} poses), {a.fit_res}^3, degree 1, after {a.steps} steps")
    baked = volume.bake_volume(model, bounds, a.fit_res, 1, attributes=())
    say(f"   as baked: {held_out_psnr(baked, small, test_poses, test, a.far):.2f} dB (train poses {held_out_psnr(baked, small, train_poses, train, a.far):.2f} dB)")
    say(f"   the sweep, a factor of 10 either side of the defaults lr_sigma = {volume.LR_SIGMA:g}, lr_coeff = {volume.LR_COEFF:g}:")
    best = None
    for ls in (0.1 * volume.LR_SIGMA, volume.LR_SIGMA, 10 * volume.LR_SIGMA):
        for lc in (0.1 * volume.LR_COEFF, volume.LR_COEFF, 10 * volume.LR_COEFF):
            vol = volume.RadianceVolume(baked.data.clone(), baked.bounds, 1)
            checks = volume.fit_volume(vol, train, small, train_poses, a.steps, lr_sigma=ls, lr_coeff=lc, far=a.far)
            db = held_out_psnr(vol, small, test_poses, test, a.far)
            say(f"     lr_sigma {ls:6g}  lr_coeff {lc:6g}   held-out {db:6.2f} dB   train {held_out_psnr(vol, small, train_poses, train, a.far):6.2f} dB   "
                f"last batch loss {checks[-1][1]:.3e}")
            if best is None or db > best[0]:
                best = (db, ls, lc)
    say(f"   best held-out: {best[0]:.2f} dB at lr_sigma {best[1]:g}, lr_coeff {best[2]:g}")


if __name__ == "__main__":
    main()
