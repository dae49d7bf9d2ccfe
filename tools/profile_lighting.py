"""GPU cost of the lighting module on a seeded PanoMipNeRF (default mlp_mode, default 128 samples per level): light probes
per second at several sizes, field_irradiance points per second, an irradiance volume end to end, and the three
lighting kernels alone with their bytes and FLOPs for the roofline comparison.  Wall times are synchronised medians
after a warm-up call.  One process per measurement so that a kernel trace holds one workload only:

    python tools/profile_lighting.py --what probes --size 32x64 [--probes 256]      # JSON line
    python tools/profile_lighting.py --what field [--points 1000000]
    python tools/profile_lighting.py --what volume                                   # 16 x 16 x 8 at 16 x 32
    python tools/profile_lighting.py --what kernels
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/profile_lighting.py --what kernels --iters 3
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
from pano_nerf_amd import lighting  # noqa: E402


def setup():
    model = pn.PanoMipNeRF(rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    model.mlp.load_state_dict(orc.init_params(4, 5))
    return model.cuda()


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("probes", "field", "volume", "kernels"), required=True)
    ap.add_argument("--size", default="32x64")
    ap.add_argument("--probes", type=int, default=256)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g)
    out = dict(what=a.what, iters=a.iters)
    if a.what in ("probes", "field", "volume"):
        model = setup()
        out.update(mlp_mode=model.mlp_mode, num_samples=model.num_samples)
    if a.what == "probes":
        H, W = (int(s) for s in a.size.split("x"))
        pos = (rnd(a.probes, 3) - 0.5) * 2.0
        sec, _ = timed(lambda: lighting.light_probes(model, pos, H, W), a.iters)
        rows = a.probes * H * W * 2 * model.num_samples
        out.update(size=[H, W], probes=a.probes, seconds=sec, probes_per_s=a.probes / sec, ms_per_probe=1e3 * sec / a.probes,
                   mlp_rows_per_s=rows / sec)
    elif a.what == "field":
        pts = (rnd(a.points, 3) - 0.5) * 2.0
        n = torch.nn.functional.normalize(rnd(a.points, 3) - 0.5, dim=-1)
        env = pn.generate_lit_rays(10, 0.01)
        sec, _ = timed(lambda: lighting.field_irradiance(model, pts, n, env), a.iters)
        out.update(points=a.points, seconds=sec, points_per_s=a.points / sec, mlp_rows_per_s=a.points * 100 / sec)
    elif a.what == "volume":
        bounds, res = ((-1.0, -0.5, -1.0), (1.0, 0.5, 1.0)), (16, 16, 8)
        sec, vol = timed(lambda: lighting.irradiance_volume(model, bounds, res, 16, 32), a.iters)
        pts = (rnd(a.points, 3) - 0.5) * 2.0
        n = torch.nn.functional.normalize(rnd(a.points, 3) - 0.5, dim=-1)
        ms = event_ms(lambda: lighting.sample_irradiance(vol, pts, n), 10)
        out.update(resolution=res, probe=[16, 32], seconds=sec, probes_per_s=16 * 16 * 8 / sec,
                   sample_points=a.points, sample_ms=ms, sample_points_per_s=a.points / (ms * 1e-3))
    else:  # the kernels alone, on synthetic probes
        res = {}
        P, H, W = 256, 64, 128
        probes = (rnd(P, H, W, 3) * 2.0).permute(0, 3, 1, 2)
        ms = event_ms(lambda: lighting.sh_project(probes), 10 * a.iters)
        byts = P * H * W * 12 + H * W * 16  # radiance once, direction table once (fp32)
        res["pn_probe_sh"] = dict(P=P, H=H, W=W, call_ms=ms, bytes=byts, tb_per_s=byts / (ms * 1e-3) / 1e12)
        P, H, W, K = 16, 128, 256, 32 * 64
        probes = (rnd(P, H, W, 3) * 2.0).permute(0, 3, 1, 2)
        nrm = torch.nn.functional.normalize(rnd(K, 3) - 0.5, dim=-1)
        ms = event_ms(lambda: lighting.irradiance(probes, nrm), a.iters)
        flops = P * K * H * W * 12  # dot 5, clamp 1, 3 multiply-adds 6
        res["pn_probe_irradiance"] = dict(P=P, H=H, W=W, K=K, call_ms=ms, flops=flops, tflop_per_s=flops / (ms * 1e-3) / 1e12)
        sh = torch.randn(16, 16, 8, 9, 3, device="cuda", generator=g)
        vol = lighting.IrradianceVolume(sh, (-1.0, -1.0, -1.0), (2.0 / 15, 2.0 / 15, 2.0 / 7))
        M = a.points
        pts = (rnd(M, 3) - 0.5) * 2.0
        n = torch.nn.functional.normalize(rnd(M, 3) - 0.5, dim=-1)
        ms = event_ms(lambda: lighting.sample_irradiance(vol, pts, n), 10 * a.iters)
        res["pn_sh_volume_irradiance"] = dict(M=M, call_ms=ms, points_per_s=M / (ms * 1e-3))
        out.update(kernels=res)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
