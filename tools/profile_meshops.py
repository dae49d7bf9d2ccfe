"""GPU cost of cleaning and simplifying a mesh (pano_nerf_amd.meshops).  One process, one JSON line:

1. The mesh: marching_tetrahedra at --res^3 of an analytic volume - a sphere of radius 0.8 with a sinusoidal relief and
   --debris small spheres (radius 2 to 4 grid steps) scattered around it, i.e. one big component and a cloud of floaters.
2. filter_components(min_faces=...) and simplify_mesh(cell = 2 and 4 grid steps) on it: the median of --iters synchronised
   calls after one warm-up call, host clock around a device synchronise (the calls hold host synchronisations of their own:
   the totals that size their outputs).  Then the same calls once more with every entry point of the library bracketed
   by a device synchronise: the time inside each HIP entry point, the rest being torch's sorts, scans and gathers.
3. Next to them, in the same run: marching_tetrahedra of that volume, and density_grid / extract_mesh of a seeded
   PanoMipNeRF on the same grid (tools/profile_geometry.py's model and box; the level is the 0.995 quantile of sigma on a
   64^3 grid): the yardsticks a fraction of which the clean-up should cost.

    python tools/profile_meshops.py [--res 256 512] [--debris 200] [--iters 3]

The resource report of the kernels comes from the compiler, not from a run:
    PN_EXTRA=-Rpass-analysis=kernel-resource-usage bash pano-nerf_amd/csrc/build.sh 2>&1 | grep -A9 "k_comp_\\|k_cluster_\\|k_mesh_"
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
from pano_nerf_amd import _lib, geometry, meshops  # noqa: E402
from tools.profile_geometry import timed  # noqa: E402

BOUNDS = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def volume(res, debris, seed=0):
    """R - |p| with a relief, and the union (max) with `debris` small spheres: positive inside"""
    dev = torch.device("cuda")
    x = torch.linspace(-1.0, 1.0, res, device=dev)
    h = 2.0 / (res - 1)
    vol = torch.empty(res, res, res, device=dev)
    slab = max(1, (1 << 24) // (res * res))
    for i in range(0, res, slab):  # in slabs: the temporaries of a 512^3 expression would not be small
        gx, gy, gz = torch.meshgrid(x[i:i + slab], x, x, indexing="ij")
        r = torch.sqrt(gx * gx + gy * gy + gz * gz)
        v = 0.8 + 0.02 * torch.sin(9.0 * gx) * torch.sin(7.0 * gy) * torch.sin(8.0 * gz) - r
        x_lo, x_hi = -1.0 + i * h, -1.0 + (min(i + slab, res) - 1) * h
        rng = np.random.RandomState(seed)  # the same debris for every slab
        for _ in range(debris):
            c = rng.uniform(-0.95, 0.95, 3)
            rad = rng.uniform(2.0, 4.0) * h
            if np.linalg.norm(c) < 0.85 + rad or c[0] + rad < x_lo - h or c[0] - rad > x_hi + h:
                continue  # it would touch the big sphere, or lies outside this slab
            d = torch.sqrt((gx - c[0]) ** 2 + (gy - c[1]) ** 2 + (gz - c[2]) ** 2)
            v = torch.maximum(v, rad - d)
        vol[i:i + slab] = v
    return vol


class EntryClock:
    """brackets every _lib.call with a device synchronise and sums the seconds per entry point"""

    def __init__(self):
        self.real, self.sec = _lib.call, {}

    def __enter__(self):
        def call(name, *args):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.real(name, *args)
            torch.cuda.synchronize()
            self.sec[name] = self.sec.get(name, 0.0) + time.perf_counter() - t0

        _lib.call = call
        return self

    def __exit__(self, *exc):
        _lib.call = self.real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--debris", type=int, default=200)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--min-faces", type=int, default=2000)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    out = dict(debris=a.debris, iters=a.iters, min_faces=a.min_faces)
    model = level = None
    if not a.skip_model:
        model = pn.PanoMipNeRF(num_samples=16, rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
        model.mlp.load_state_dict(orc.init_params(4, 5))
        model = model.cuda()
        level = float(torch.quantile(geometry.density_grid(model, BOUNDS, 64).view(-1).float(), 0.995))
        out["level"], out["mlp_mode"] = level, model.mlp_mode
    for res in a.res:
        h = 2.0 / (res - 1)
        vol = volume(res, a.debris)
        sec, (v, f) = timed(lambda: geometry.marching_tetrahedra(vol, 0.0, BOUNDS), a.iters)
        out[f"marching_tetrahedra_{res}_s"] = sec
        out[f"mesh_{res}_vertices"], out[f"mesh_{res}_faces"] = int(v.shape[0]), int(f.shape[0])
        del vol
        mesh = geometry.Mesh(v, f, None, None)
        sec, (clean, _, _) = timed(lambda: meshops.filter_components(mesh, min_faces=a.min_faces), a.iters)
        out[f"filter_{res}_s"], out[f"filter_{res}_faces_left"] = sec, int(clean.faces.shape[0])
        out[f"components_{res}"] = meshops.mesh_components(f, int(v.shape[0]))[2]
        with EntryClock() as clock:
            meshops.filter_components(mesh, min_faces=a.min_faces)
        out[f"filter_{res}_entry_points_s"] = clock.sec
        for cells in (2, 4):
            sec, (small, _, _, flags) = timed(lambda: meshops.simplify_mesh(clean, cell=cells * h), a.iters)
            key = f"simplify_{res}_{cells}h"
            out[f"{key}_s"], out[f"{key}_faces"], out[f"{key}_vertices"] = sec, int(small.faces.shape[0]), int(small.vertices.shape[0])
            out[f"{key}_fallbacks"] = int((flags == 1).sum())
            out[f"{key}_edges"] = meshops.edge_counts(small.faces)
            with EntryClock() as clock:
                meshops.simplify_mesh(clean, cell=cells * h)
            out[f"{key}_entry_points_s"] = clock.sec
        sec, (small, _, _, _, info) = timed(lambda: meshops.simplify_mesh(clean, target_faces=20000, return_info=True), 1)
        out[f"target20000_{res}_s"], out[f"target20000_{res}_faces"], out[f"target20000_{res}_cell_over_h"] = \
            sec, int(small.faces.shape[0]), info["cell"] / h
        del mesh, clean, small, v, f
        if model is not None:
            sec, sigma = timed(lambda: geometry.density_grid(model, BOUNDS, res), 1)
            out[f"density_grid_{res}_s"] = sec
            del sigma
            try:
                sec, m = timed(lambda: geometry.extract_mesh(model, BOUNDS, res, level, colors=None), 1)
                out[f"extract_mesh_{res}_s"], out[f"extract_mesh_{res}_faces"] = sec, int(m.faces.shape[0])
                del m
            except (RuntimeError, torch.cuda.OutOfMemoryError) as e:  # a noise field can have too many faces to hold
                out[f"extract_mesh_{res}_s"], out[f"extract_mesh_{res}_error"] = None, str(e)[:120]
        torch.cuda.empty_cache()
        print(json.dumps({k: out[k] for k in out if f"_{res}" in k}), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
