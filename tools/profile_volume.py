"""GPU cost of the baked radiance volume (pano_nerf_amd.volume).  One process, one JSON line:

1. bake_volume of a seeded PanoMipNeRF at 128^3 and 256^3 (sh_degree 1, albedo + normal, default sigma_min), split into
   sigma (density_grid alone), colour (bake_volume minus density_grid: the compaction, D = 16 query_field sweeps, the fit
   and the attributes) and occupancy (pn_volume_occupancy between device events).
2. render_volume of a 480 x 640 pinhole frame and a 512 x 1024 panorama from the middle of the box, skip on and off, at
   two occupancy levels of the 256^3 volume (the default bake, and the same volume emptied outside a ball), between
   device events; next to render_view of the same frames (host clock around a device synchronise).  The diagnostic "taps"
   output counts the samples, from which the gathered bytes follow: 8 corners x 4 B for every sigma tap and 8 x 4 x 3 K B
   more for every sample with sigma > 0 (rgb and depth are asked for, so the attribute channels are not read).
3. volume_probes at 32 x 64 next to lighting.light_probes at the same positions.
4. The HBM copy rate of this run (a 1 GiB device-to-device copy: bytes read plus bytes written over its time).

    python tools/profile_volume.py [--res 128 256] [--probes 64] [--window 5]

The resource report of the kernels comes from the compiler, not from a run:
    PN_EXTRA=-Rpass-analysis=kernel-resource-usage bash pano-nerf_amd/csrc/build.sh 2>&1 | grep -A9 k_volume
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pano_nerf_amd import geometry, lighting, views, volume  # noqa: E402
from tools.profile_fusion import setup  # noqa: E402
from tools.profile_geometry import timed  # noqa: E402
from tools.profile_textures import windowed  # noqa: E402


def copy_rate():
    """TB/s of a 1 GiB device copy, read plus written bytes"""
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    ms = windowed(lambda: dst.copy_(src), 10)
    return 2.0 * src.numel() * 4 / (1e-3 * ms) / 1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--probes", type=int, default=64)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--far", type=float, default=10.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_volume.py measures on a HIP device; none is visible")
    model, bounds, _ = setup()
    lo, hi = (np.asarray(c) for c in bounds)
    out = dict(bounds=bounds, window=a.window, mlp_mode=model.mlp_mode, num_samples=model.num_samples, far=a.far)
    out["hbm_copy_TB_s"] = copy_rate()

    vol = None
    for res in a.res:
        sec_sigma, _ = timed(lambda: geometry.density_grid(model, bounds, res), 2)
        sec_bake, vol = timed(lambda: volume.bake_volume(model, bounds, res), 2)
        out[f"bake_{res}_sigma_s"], out[f"bake_{res}_colour_s"] = sec_sigma, sec_bake - sec_sigma
        out[f"bake_{res}_occupancy_ms"] = windowed(vol.refresh, a.window)
        out[f"bake_{res}_kept_vertices"] = float((vol.sigma > 0).float().mean())
        out[f"bake_{res}_occupied_bricks"] = float(vol.occupancy.float().mean())
        out[f"bake_{res}_MB"] = vol.data.numel() * 4 / 1e6

    # two occupancy levels of the last (largest) volume: as baked, and the same volume emptied outside a ball in front of
    # the pinhole camera (an object in an empty room: most bricks unoccupied)
    pose = np.eye(4)
    pose[:3, 3] = 0.5 * (lo + hi)
    ext = hi - lo
    centre = pose[:3, 3] + np.array([0.0, 0.0, -0.3 * ext[2]])
    mean = geometry.grid_points(bounds, vol.resolution, 0.0, "cuda")[0]
    ball = ((mean - torch.tensor(centre, device="cuda", dtype=torch.float32)) ** 2).sum(1) < (0.15 * float(ext.min())) ** 2
    sparse = volume.RadianceVolume((vol.data.view(-1, vol.channels) * ball[:, None]).view(vol.data.shape).contiguous(),
                                   vol.bounds, vol.sh_degree, vol._attrs)
    del mean, ball
    levels = {"baked": vol, "ball": sparse}
    cams = {"pinhole_480x640": views.perspective_camera(480, 640, fov_x_deg=70.0), "pano_512x1024": views.pano_camera(512, 1024)}
    K = (vol.sh_degree + 1) ** 2
    for tag, cam in cams.items():
        sec, _ = timed(lambda: views.render_view(model, cam, pose, outputs=("rgb", "depth"), far=a.far), 2)
        out[f"{tag}_render_view_s"] = sec
        rays = views.generate_camera_rays(cam, pose, 0.0, a.far, "cuda")
        for level, v in levels.items():
            out[f"{level}_kept_vertices"] = float((v.sigma > 0).float().mean())
            out[f"{level}_occupied_bricks"] = float(v.occupancy.float().mean())
            for skip in (True, False):
                key = f"{tag}_{level}_{'skip' if skip else 'noskip'}"
                ms = windowed(lambda: volume.render_volume(v, cam, pose, ("rgb", "depth"), 0.0, a.far, skip=skip), a.window)
                taps = volume.march_rays(v, rays.origins, rays.directions, rays.near, rays.far, skip=skip,
                                         outputs=("taps",))["taps"].sum(0).tolist()
                # render_volume asks for rgb and depth only: the attribute channels are not read
                gathered = 32.0 * taps[0] + 32.0 * 3 * K * taps[1]
                out[f"{key}_ms"], out[f"{key}_speedup_vs_render_view"] = ms, sec / (1e-3 * ms)
                out[f"{key}_sigma_taps"], out[f"{key}_colour_taps"] = taps
                out[f"{key}_gathered_TB_s"] = gathered / (1e-3 * ms) / 1e12
                out[f"{key}_share_of_copy_rate"] = out[f"{key}_gathered_TB_s"] / out["hbm_copy_TB_s"]

    g = torch.Generator(device="cuda").manual_seed(0)
    pos = torch.tensor(lo + 0.25 * (hi - lo), device="cuda", dtype=torch.float32) + \
        torch.rand(a.probes, 3, device="cuda", generator=g) * torch.tensor(0.5 * (hi - lo), device="cuda", dtype=torch.float32)
    sec_l, _ = timed(lambda: lighting.light_probes(model, pos, 32, 64, 0.0, a.far), 2)
    ms_v = windowed(lambda: volume.volume_probes(vol, pos, 32, 64, 0.0, a.far), a.window)
    out["light_probes_per_s"], out["volume_probes_per_s"] = a.probes / sec_l, a.probes / (1e-3 * ms_v)
    out["volume_probes_ms"] = ms_v
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
