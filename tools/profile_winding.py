"""GPU cost of winding-number queries (pano_nerf_amd.winding).  One process, one run; writes a text report (default
profiles/geometry_winding.txt) and prints the same figures as one JSON line.

1. winding_number against icospheres of 1 280, 81 920 and 1 310 720 faces (levels 3, 6, 8; radius 0.35) with --points query
   points (default 2^20) of tools/profile_meshdist.py's two kinds: "near" the surface and spread through the "box".  The
   Barnes-Hut walk at beta = 2, 4, 8 with the tree and the moments made beforehand (MeshBVH.build and the moments pass are
   timed on their own), its largest distance from brute force on the points brute force was run on, and the visits per
   point, counted by tests/_winding_ref.py's walk over the device's own nodes and moments on the first --visit-points points
   of each kind.  Brute force visits P x F pairs: it is run on all points while P x F <= --brute-pairs, otherwise on the
   first P' = brute-pairs / F points, and the report says so.
2. Next to each figure, in the same run: closest_point(accel=<the same tree>) on the same points.
3. signed_distance_grid and remesh at 128^3 of a simplified marching-tetrahedra mesh (tools/profile_meshops.py's volume at
   --res, debris filtered, simplify_mesh at 2 grid steps).

Times are medians of --iters synchronised calls after one warm-up call, host clock around a device synchronise, with the
spread (max - min) of the repeats.  The resource report of the kernels comes from the compiler, not from a run:
    PN_EXTRA=-Rpass-analysis=kernel-resource-usage bash pano-nerf_amd/csrc/build.sh 2>&1 | grep -A9 "k_winding\\|k_bvh_moments"
PN_LIB=<another build of the library> in the environment measures that build, as tools/profile_conventions.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pano_nerf_amd import _lib, geometry, meshdist, meshops, objects, winding  # noqa: E402

if os.environ.get("PN_LIB"):  # another build of the library, as tools/profile_conventions.py
    _lib.LIB_PATH = os.path.abspath(os.environ["PN_LIB"])
from tools.profile_meshdist import BOUNDS, CENTRE, RADIUS, icosphere, query_sets, timed  # noqa: E402

BETAS = (2.0, 4.0, 8.0)


def fresh_moments(tree, tv, tf):
    tree._winding_moments = None
    return winding._moments(tree, tv, tf, tv.device)


def winding_rows(level, P, iters, brute_pairs, visit_points, out, lines):
    import _winding_ref as ref
    dev = torch.device("cuda")
    v, f = icosphere(level, RADIUS, CENTRE)
    tv, tf = torch.as_tensor(v).to(dev), torch.as_tensor(f).to(dev)
    F = int(tf.shape[0])
    ms, sp, tree = timed(lambda: objects.MeshBVH.build(tv, tf), iters)
    mms, msp, mom = timed(lambda: fresh_moments(tree, tv, tf), iters)
    out[f"build_{F}_ms"], out[f"moments_{F}_ms"] = ms, mms
    lines.append(f"  {F:>9,d} faces   MeshBVH.build {ms:8.3f} ms (+- {sp:.3f})   pn_bvh_moments {mms:8.3f} ms (+- {msp:.3f})")
    nodes, mom_h = tree.nodes.cpu().numpy(), mom.cpu().numpy()
    Pb = P if P * F <= brute_pairs else max(int(brute_pairs // F) // 256 * 256, 256)
    for kind, pts in query_sets(tv, tf, P).items():
        key = f"winding_{F}_{kind}"
        bms, bsp, brute = timed(lambda: winding.winding_number(pts[:Pb], tv, tf, accel=None), max(1, min(iters, 2)))
        cms, csp, _ = timed(lambda: meshdist.closest_point(pts, tv, tf, accel=tree), iters)
        out[f"{key}_brute_ms"], out[f"{key}_brute_points"], out[f"{key}_closest_point_bvh_ms"] = bms, Pb, cms
        lines.append(f"    {kind:4s} brute force on {Pb:,d} points{'' if Pb == P else ' (P x F above the limit: a part of the points)'} "
                     f"{bms:10.3f} ms (+- {bsp:.3f}) = {1e6 * bms / Pb:10.3f} ns/point = {1e9 * bms / Pb / F:6.3f} ps/pair   "
                     f"closest_point(bvh) on {P:,d} points {cms:9.3f} ms (+- {csp:.3f})")
        host_pts = pts[:visit_points].cpu().numpy()
        for beta in BETAS:
            wms, wsp, walk = timed(lambda: winding.winding_number(pts, tv, tf, accel=tree, beta=beta), iters)
            err = float((walk[:Pb].double() - brute.double()).abs().max())
            flips = int(((walk[:Pb] > 0.5) != (brute > 0.5)).sum())
            visits = ref.walk(host_pts, v, f, nodes, mom_h, beta)["visits"]
            out[f"{key}_beta{beta:g}"] = dict(ms=wms, spread_ms=wsp, max_err=err, inside_flips=flips,
                                              visits_mean=float(visits.mean()), visits_max=int(visits.max()))
            lines.append(f"         walk beta {beta:g}: {P:,d} points {wms:9.3f} ms (+- {wsp:.3f}) = {1e6 * wms / P:8.3f} ns/point   "
                         f"visits/point {visits.mean():7.1f} (max {visits.max()}, of {len(host_pts)} points) = "
                         f"{1e6 * wms / P / visits.mean():6.3f} ns/visit   brute / walk per point {(bms / Pb) / (wms / P):8.1f}   "
                         f"max |w - w_brute| {err:.3e}, inside differs at {flips}")
    del tree


def export_rows(res, iters, out, lines):
    from tools.profile_meshops import volume
    h = 2.0 / (res - 1)
    v, f = geometry.marching_tetrahedra(volume(res, 200), 0.0, BOUNDS)
    mesh = meshops.filter_components(geometry.Mesh(v, f, None, None), min_faces=2000)[0]
    small = meshops.simplify_mesh(mesh, cell=2 * h)[0]
    F = int(small.faces.shape[0])
    n = 128
    out.update(export_res=res, export_faces=F)
    lines.append(f"  the {res}^3 marching-tetrahedra mesh, debris filtered, simplify_mesh(cell = 2 h): {F:,d} faces; beta = "
                 f"{winding.DEFAULT_BETA:g}, one tree per call (built inside the timed call):")
    for name, fn in (("signed_distance_grid", lambda: winding.signed_distance_grid(small, BOUNDS, n)),
                     ("distance_grid", lambda: meshdist.distance_grid(small, BOUNDS, n)),
                     ("winding_grid", lambda: winding.winding_grid(small, BOUNDS, n)),
                     ("remesh", lambda: winding.remesh(small, n, BOUNDS))):
        ms, sp, res_ = timed(fn, iters)
        out[f"export_{name}_ms"] = ms
        extra = ""
        if name == "remesh":
            extra = f"   -> {int(res_.faces.shape[0]):,d} faces, edges {meshops.edge_counts(res_.faces)}"
        lines.append(f"    {name:22s} at {n}^3 {ms:9.3f} ms (+- {sp:.3f}){extra}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, nargs="+", default=[3, 6, 8])
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--brute-pairs", type=float, default=1e10)
    ap.add_argument("--visit-points", type=int, default=512)
    ap.add_argument("--res", type=int, default=256, help="grid of the exported mesh; 0 skips it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_winding.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/profile_winding.py measures on the GPU: no device found")
    out = dict(points=a.points, iters=a.iters, brute_pairs=a.brute_pairs, device=torch.cuda.get_device_name(0))
    lines = [f"Winding-number queries on one {out['device']}, tools/profile_winding.py (--levels {' '.join(map(str, a.levels))} "
             f"--points {a.points} --iters {a.iters} --brute-pairs {a.brute_pairs:g} --visit-points {a.visit_points} --res {a.res}; "
             "one process, one run).",
             f"Times: median of {a.iters} synchronised calls after one warm-up call (brute force: of at most 2), host clock "
             "around a device synchronise, (+- max - min of the repeats).", "",
             "winding_number against icospheres of radius 0.35 (\"near\": surface samples pushed off by N(0, (0.01 R)^2) along the "
             "normal; \"box\": uniform within 1.5 R), tree and moments made beforehand; closest_point on the same tree and points "
             "is the yardstick:"]
    for level in a.levels:
        winding_rows(level, a.points, a.iters, a.brute_pairs, a.visit_points, out, lines)
        torch.cuda.empty_cache()
    if a.res:
        lines.append("")
        export_rows(a.res, a.iters, out, lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    sys.stderr.write(text)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
