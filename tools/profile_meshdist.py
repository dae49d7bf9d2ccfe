"""GPU cost of mesh distance queries (pano_nerf_amd.meshdist).  One process, one run; writes a text report (default
profiles/geometry_meshdist.txt) and prints the same figures as one JSON line.

1. closest_point against icospheres of 1 280, 81 920 and 1 310 720 faces (levels 3, 6, 8; radius 0.35) with --points query
   points (default 2^20) of two kinds: "near" = surface samples of the mesh pushed off it by a seeded normal offset of 1 % of
   the radius (what compare_meshes asks), and "box" = uniform in the box of 1.5 radii around it.  The BVH walk with the tree
   built beforehand (the build is timed on its own), and brute force.  Brute force visits P x F pairs: it is run on all
   points while P x F <= --brute-pairs (default 3e10), otherwise on the first P' = brute-pairs / F points, and the report
   says so and gives the time per point for both.
2. Next to each figure, in the same run: trace_mesh(accel=<the same tree>) on the same number of rows - rays from the
   query points towards the sphere's centre - the yardstick the issue names.
3. compare_meshes of a 512^3-grid marching-tetrahedra mesh (tools/profile_meshops.py's volume, debris filtered) against its
   simplify_mesh result at 2 grid steps, default samples, with its stages timed on their own.

Times are medians of --iters synchronised calls after one warm-up call, host clock around a device synchronise, with the
spread (max - min) of the repeats.  The resource report of the kernels comes from the compiler, not from a run:
    PN_EXTRA=-Rpass-analysis=kernel-resource-usage bash pano-nerf_amd/csrc/build.sh 2>&1 | grep -A9 "k_closest\\|k_face_\\|k_sample"
PN_LIB=<another build of the library> in the environment measures that build, as tools/profile_conventions.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pano_nerf_amd import _lib, geometry, meshdist, meshops, objects  # noqa: E402

if os.environ.get("PN_LIB"):  # another build of the library, as tools/profile_conventions.py
    _lib.LIB_PATH = os.path.abspath(os.environ["PN_LIB"])

RADIUS, CENTRE = 0.35, (0.5, -0.1, 0.8)
BOUNDS = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def icosphere(level, radius, centre):
    """tools/profile_objects.py's icosphere, subdivided with numpy (level 8 has 1.3 M faces)"""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1),
                  (p, 0, 1), (-p, 0, -1), (-p, 0, 1)], np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
                  (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
                  (9, 8, 1)], np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(level):
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        key = np.minimum(e[:, 0], e[:, 1]) * len(v) + np.maximum(e[:, 0], e[:, 1])
        uniq, inv = np.unique(key, return_inverse=True)
        m = v[uniq // len(v)] + v[uniq % len(v)]
        mid = (len(v) + inv).reshape(3, -1)  # ab, bc, ca per face
        v = np.concatenate([v, m / np.linalg.norm(m, axis=1, keepdims=True)])
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        ab, bc, ca = mid
        f = np.concatenate([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1), np.stack([ab, bc, ca], 1)])
    return (v * radius + np.asarray(centre)).astype(np.float32), f.astype(np.int32)


def timed(fn, iters):
    """(median ms, max - min ms, the last result)"""
    out = fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * (max(t) - min(t)), out


def query_sets(tv, tf, P, seed=0):
    dev = tv.device
    g = torch.Generator(device=dev).manual_seed(seed)
    pts, _, _ = meshdist.sample_surface((tv, tf), P)
    c = torch.tensor(CENTRE, device=dev)
    n = torch.nn.functional.normalize(pts - c, dim=1)
    near = (pts + n * (0.01 * RADIUS) * torch.randn(P, 1, device=dev, generator=g)).contiguous()
    box = (c + 1.5 * RADIUS * (2.0 * torch.rand(P, 3, device=dev, generator=g) - 1.0)).contiguous()
    return {"near": near, "box": box}


def closest_rows(level, P, iters, brute_pairs, out, lines):
    dev = torch.device("cuda")
    v, f = icosphere(level, RADIUS, CENTRE)
    tv, tf = torch.as_tensor(v).to(dev), torch.as_tensor(f).to(dev)
    F = int(tf.shape[0])
    ms, sp, tree = timed(lambda: objects.MeshBVH.build(tv, tf), iters)
    out[f"build_{F}_ms"] = ms
    lines.append(f"  {F:>9,d} faces   MeshBVH.build {ms:8.3f} ms (+- {sp:.3f})")
    c = torch.tensor(CENTRE, device=dev)
    for kind, pts in query_sets(tv, tf, P).items():
        ms, sp, walk = timed(lambda: meshdist.closest_point(pts, tv, tf, accel=tree), iters)
        dirs = (c - pts).contiguous()
        tms, tsp, hit = timed(lambda: objects.trace_mesh(pts, dirs, tv, tf, accel=tree), iters)
        Pb = P if P * F <= brute_pairs else max(int(brute_pairs // F) // 256 * 256, 256)
        bms, bsp, brute = timed(lambda: meshdist.closest_point(pts[:Pb], tv, tf, accel=None), max(1, min(iters, 2)))
        same = all(torch.equal(a[:Pb].view(torch.int32) if a.dtype == torch.float32 else a[:Pb],
                               b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(walk, brute))
        key = f"closest_{F}_{kind}"
        out[f"{key}_bvh_ms"], out[f"{key}_bvh_spread_ms"], out[f"{key}_trace_bvh_ms"] = ms, sp, tms
        out[f"{key}_brute_ms"], out[f"{key}_brute_points"], out[f"{key}_bvh_equals_brute"] = bms, Pb, bool(same)
        out[f"{key}_trace_hits"] = int((hit[1] >= 0).sum())
        lines.append(f"    {kind:4s} {P:,d} points   BVH walk {ms:9.3f} ms (+- {sp:.3f}) = {1e6 * ms / P:7.3f} ns/point   "
                     f"trace_mesh(bvh), {P:,d} rays, {out[key + '_trace_hits']:,d} hits {tms:9.3f} ms (+- {tsp:.3f})")
        lines.append(f"         brute force on {Pb:,d} points{'' if Pb == P else ' (P x F above the limit: a part of the points)'} "
                     f"{bms:10.3f} ms (+- {bsp:.3f}) = {1e6 * bms / Pb:10.3f} ns/point   BVH / brute force per point "
                     f"1 : {(bms / Pb) / (ms / P):.1f}   same bits on those points: {same}")
    del tree


def compare_rows(res, iters, out, lines):
    from tools.profile_meshops import volume
    h = 2.0 / (res - 1)
    v, f = geometry.marching_tetrahedra(volume(res, 200), 0.0, BOUNDS)
    mesh = meshops.filter_components(geometry.Mesh(v, f, None, None), min_faces=2000)[0]
    small = meshops.simplify_mesh(mesh, cell=2 * h)[0]
    Fa, Fb = int(mesh.faces.shape[0]), int(small.faces.shape[0])
    ms, sp, s = timed(lambda: meshdist.compare_meshes(small, mesh), iters)
    out.update(compare_res=res, compare_faces=(Fb, Fa), compare_ms=ms, compare_spread_ms=sp,
               compare_scores={k: s[k] for k in ("accuracy", "completeness", "chamfer", "hausdorff", "normal_consistency",
                                                 "thresholds", "precision", "recall", "fscore", "samples")})
    lines.append(f"  compare_meshes(simplify_mesh(cell = 2 h) [{Fb:,d} f], the {res}^3 mesh [{Fa:,d} f]), {s['samples']:,d} samples "
                 f"per mesh: {ms:.3f} ms (+- {sp:.3f})")
    n = s["samples"]
    samples = {}
    for name, m in (("simplified", small), ("original", mesh)):
        a, asp, (samples[name], _, _) = timed(lambda: meshdist.sample_surface(m, n), iters)
        out[f"compare_{name}_sample_surface_ms"] = a
        lines.append(f"    {name:10s} sample_surface {a:7.3f} ms (+- {asp:.3f})")
    for name, m, other in (("simplified", small, "original"), ("original", mesh, "simplified")):
        b, bsp, tree = timed(lambda: objects.MeshBVH.build(m.vertices, m.faces), iters)
        c, csp, _ = timed(lambda: meshdist.closest_point(samples[other], m.vertices, m.faces, accel=tree), iters)
        out[f"compare_{name}_stages_ms"] = dict(bvh_build=b, closest_point_of_the_others_samples=c)
        lines.append(f"    {name:10s} MeshBVH.build {b:7.3f} ms (+- {bsp:.3f})   closest_point of the {other} mesh's samples against "
                     f"it, tree given {c:7.3f} ms (+- {csp:.3f})")
    lines.append(f"    scores (scene units; the box is [-1, 1]^3, h = {h:.5f}): accuracy {s['accuracy']:.6f}  completeness "
                 f"{s['completeness']:.6f}  chamfer {s['chamfer']:.6f}  hausdorff {s['hausdorff']:.6f}  (sqrt(3) cell = "
                 f"{np.sqrt(3.0) * 2 * h:.6f})")
    lines.append(f"    tau {s['thresholds']}: precision {tuple(round(x, 4) for x in s['precision'])}  recall "
                 f"{tuple(round(x, 4) for x in s['recall'])}  fscore {tuple(round(x, 4) for x in s['fscore'])}  normal consistency "
                 f"{s['normal_consistency']:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, nargs="+", default=[3, 6, 8])
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--brute-pairs", type=float, default=3e10)
    ap.add_argument("--res", type=int, default=512, help="grid of the compare_meshes mesh; 0 skips it")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "geometry_meshdist.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/profile_meshdist.py measures on the GPU: no device found")
    out = dict(points=a.points, iters=a.iters, brute_pairs=a.brute_pairs, device=torch.cuda.get_device_name(0))
    lines = [f"Mesh distance queries on one {out['device']}, tools/profile_meshdist.py (--levels {' '.join(map(str, a.levels))} "
             f"--points {a.points} --iters {a.iters} --brute-pairs {a.brute_pairs:g} --res {a.res}; one process, one run).",
             f"Times: median of {a.iters} synchronised calls after one warm-up call (brute force: of at most 2), host clock "
             "around a device synchronise, (+- max - min of the repeats).", "",
             "closest_point against icospheres of radius 0.35 (\"near\": surface samples pushed off by N(0, (0.01 R)^2) along the "
             "normal; \"box\": uniform within 1.5 R), tree built beforehand; trace_mesh on the same tree and row count (rays from "
             "the points towards the centre) is the yardstick:"]
    for level in a.levels:
        closest_rows(level, a.points, a.iters, a.brute_pairs, out, lines)
        torch.cuda.empty_cache()
    if a.res:
        lines.append("")
        compare_rows(a.res, a.iters, out, lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    sys.stderr.write(text)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
