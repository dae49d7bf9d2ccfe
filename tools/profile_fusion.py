"""GPU cost of TSDF fusion (pano_nerf_amd.fusion).  One process, one JSON line:

1. TSDFVolume.integrate of 32 panorama views of 256 x 512 and of 32 pinhole views of 480 x 640 into 256^3 and 512^3
   volumes: the mean of --window back-to-back calls between two device events (one warm-up call), and the (voxel, view)
   pairs per second that makes.  The depth images are render_view's fine_dep of a seeded PanoMipNeRF (default mode,
   128 + 128 samples) at 32 poses on a circle inside the box; the kernel's work does not depend on their values (every
   voxel projects into every view whatever the depth says), only the gather's addresses do.
2. Next to them, in the same run: the render_view(outputs=("depth",)) cost of those 32 views (each view once, after one
   warm-up view; host clock around a device synchronise), and density_grid + marching_tetrahedra at the same resolution
   (tools/profile_geometry.py's level: the 0.6 quantile of sigma on a 64^3 grid), the other route to a mesh.
3. mesh() and mesh(cull=True) of a volume fused from constant-depth panoramas at the same poses (occupancy +
   marching_tetrahedra + the host copy of its totals; the untrained field's own depth has no zero crossing in the box).

    python tools/profile_fusion.py [--res 256 512] [--views 32] [--window 3]

The resource report of the kernel comes from the compiler, not from a run:
    PN_EXTRA=-Rpass-analysis=kernel-resource-usage bash pano-nerf_amd/csrc/build.sh 2>&1 | grep -A9 k_tsdf_integrate
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
from pano_nerf_amd import fusion, geometry, views  # noqa: E402
from tools.profile_geometry import timed  # noqa: E402
from tools.profile_textures import windowed  # noqa: E402


def setup():
    """tools/profile_geometry.py's model, box and level, but with the renderer's default 128 + 128 samples"""
    model = pn.PanoMipNeRF(rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    model.mlp.load_state_dict(orc.init_params(4, 5))
    model = model.cuda()
    _, _, _, c2ws = orc.synthetic_scene(8, 16, 3, seed=4)
    cams = np.stack([c[:3, 3] for c in c2ws])
    bounds = (tuple((cams.min(0) - 1.0).tolist()), tuple((cams.max(0) + 1.0).tolist()))
    vol = geometry.density_grid(model, bounds, 64)
    return model, bounds, float(torch.quantile(vol.view(-1).float(), 0.6))


def circle(n, centre, radius):
    """n look-at poses on a horizontal circle around `centre`, looking across it"""
    out = []
    for a in np.linspace(0.0, 2.0 * np.pi, n, endpoint=False):
        eye = centre + radius * np.array([np.cos(a), 0.1 * np.sin(3 * a), np.sin(a)])
        out.append(views.look_at(eye, centre - 0.5 * (eye - centre)))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--window", type=int, default=3)
    ap.add_argument("--far", type=float, default=10.0)
    a = ap.parse_args()
    model, bounds, level = setup()
    lo, hi = (np.asarray(c) for c in bounds)
    poses = circle(a.views, 0.5 * (lo + hi), 0.25 * float((hi - lo).min()))
    cams = {"pano_256x512": views.pano_camera(256, 512), "pinhole_480x640": views.perspective_camera(480, 640, fov_x_deg=70.0)}
    out = dict(views=a.views, window=a.window, bounds=bounds, level=level, mlp_mode=model.mlp_mode, num_samples=model.num_samples)
    depths = {}
    for tag, cam in cams.items():
        render = lambda p: views.render_view(model, cam, p, outputs=("depth",), far=a.far)["fine_dep"]
        render(poses[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        depths[tag] = torch.cat([render(p) for p in poses])
        torch.cuda.synchronize()
        out[f"{tag}_render_view_s"] = time.perf_counter() - t0
        out[f"{tag}_rays"] = a.views * cam.h * cam.w
    for res in a.res:
        pairs = float(res) ** 3 * a.views
        for tag, cam in cams.items():
            vol = fusion.TSDFVolume(bounds, res, device="cuda")
            ms = windowed(lambda: vol.integrate(depths[tag], cam, poses, depth_max=0.98 * a.far, max_weight=64.0), a.window)
            out[f"integrate_{res}_{tag}_ms"] = ms
            out[f"integrate_{res}_{tag}_pairs_per_s"] = pairs / (1e-3 * ms)
            out[f"integrate_{res}_{tag}_share_of_render"] = 1e-3 * ms / out[f"{tag}_render_view_s"]
            out[f"integrate_{res}_{tag}_observed"] = float(vol.observed().float().mean())
            del vol
        # the untrained field's depth lies beyond the box (no zero crossing inside it), so mesh() is timed on a volume fused
        # from constant-depth panoramas at the same poses: the union of 32 spheres of radius 0.9, carved
        vol = fusion.TSDFVolume(bounds, res, device="cuda")
        vol.integrate(torch.full_like(depths["pano_256x512"], 0.9), cams["pano_256x512"], poses)
        for cull in (False, True):
            sec, (v, f) = timed(lambda: vol.mesh(cull=cull), 2)
            key = f"mesh_{res}_cull" if cull else f"mesh_{res}"
            out[f"{key}_s"], out[f"{key}_vertices"], out[f"{key}_faces"] = sec, int(v.shape[0]), int(f.shape[0])
            del v, f
        del vol
        sec_g, sigma = timed(lambda: geometry.density_grid(model, bounds, res), 2)
        sec_t, (v, f) = timed(lambda: geometry.marching_tetrahedra(sigma, level, bounds), 2)
        out[f"density_grid_{res}_s"], out[f"marching_tetrahedra_{res}_s"] = sec_g, sec_t
        out[f"marching_tetrahedra_{res}_vertices"] = int(v.shape[0])
        del sigma, v, f
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
