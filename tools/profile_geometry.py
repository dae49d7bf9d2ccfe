"""GPU cost of exporting the geometry of a seeded PanoMipNeRF (default mlp_mode): extract_mesh over a box around the
cameras of the oracle's synthetic scene, its sigma grid alone, and the training forward chain (activations kept) on the
same number of rows per launch, for the rows/s comparison.  One process per measurement so that a kernel trace holds
one workload only:

    python tools/profile_geometry.py --res 256 [--iters 5]          # wall time per call (synchronised), JSON line
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/profile_geometry.py --res 256 --iters 2 --mesh-only
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
from pano_nerf_amd import geometry, render  # noqa: E402
from pano_nerf_amd import _lib  # noqa: E402


def setup():
    model = pn.PanoMipNeRF(num_samples=16, rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    model.mlp.load_state_dict(orc.init_params(4, 5))
    model = model.cuda()
    _, _, _, c2ws = orc.synthetic_scene(8, 16, 3, seed=4)
    cams = np.stack([c[:3, 3] for c in c2ws])
    bounds = (tuple((cams.min(0) - 1.0).tolist()), tuple((cams.max(0) + 1.0).tolist()))
    vol = geometry.density_grid(model, bounds, 64)
    level = float(torch.quantile(vol.view(-1).float(), 0.6))
    return model, bounds, level


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


def train_forward_rate(model, rows, iters):
    """rows/s of the training forward chain (pn_chain_forward with the activation stash) on `rows` sample rows."""
    dev = torch.device("cuda")
    f = render._Field.of(model, dev)
    vd = torch.nn.functional.normalize(torch.randn(rows // 128, 3, device=dev), dim=-1)
    ev = f.evaluation(rows, 128, vd, True)
    ev.mean.uniform_(-1.5, 1.5)
    ev.cov.fill_(1e-4)
    sec, _ = timed(lambda: f.forward(ev), iters)
    return rows / sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--mesh-only", action="store_true", help="extract_mesh calls only (for a kernel trace)")
    a = ap.parse_args()
    model, bounds, level = setup()
    out = dict(res=a.res, mlp_mode=model.mlp_mode, level=level, bounds=bounds, iters=a.iters)
    sec, mesh = timed(lambda: pn.extract_mesh(model, bounds, a.res, level), a.iters)
    out.update(extract_mesh_s=sec, vertices=int(mesh.vertices.shape[0]), faces=int(mesh.faces.shape[0]))
    if not a.mesh_only:
        rows = a.res ** 3
        sec_g, _ = timed(lambda: geometry.density_grid(model, bounds, a.res), a.iters)
        vol = geometry.density_grid(model, bounds, a.res)
        sec_t, _ = timed(lambda: geometry.marching_tetrahedra(vol, level, bounds), a.iters)
        chunk = min(rows, geometry._CHUNK_CHAIN)
        out.update(density_grid_s=sec_g, grid_rows_per_s=rows / sec_g, marching_tetrahedra_s=sec_t,
                   train_forward_rows_per_s=train_forward_rate(model, chunk, a.iters), train_forward_rows=chunk)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
