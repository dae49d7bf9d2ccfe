"""Every output of the mesh queries that walk pn_bvh.hip's tree, from one build of the library, for a comparison of raw bits
between two builds (profiles/refactor_bvh_walk.txt, section 2).

    python tools/compare_bvh_walk.py --out new.npz
    PN_LIB=<another build of the library> python tools/compare_bvh_walk.py --out old.npz     # as tools/profile_conventions.py
    python tools/compare_bvh_walk.py --compare old.npz new.npz                               # needs no device

One process per library.  Meshes: the ones tests/test_gpu_bvh.py, test_gpu_meshdist.py and test_gpu_winding.py build (F = 1,
2, 3, ico3, soup, sliver, coincident, fan, stack, bad).  Query sets of 65 and 257 rows (neither fills its last workgroup of 64
or 256), seeded, with a NaN row and a row with an infinite component.  Per mesh and set, brute force and BVH: trace_mesh
(closest and any-hit, with and without t_max), shadow_ratio, closest_point and signed_distance (with and without
max_distance), winding_number (beta 2 and 4), and the tree's nodes and moments.  --compare counts the 32-bit words that
differ per group, NaNs by their bit patterns, and exits 1 if any does."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
f32 = np.float32


def meshes():
    import _meshdist_ref as md
    out = {f"F = {k}": md.meshes()[f"ico3[:{k}]"] for k in (1, 2, 3)}
    out.update(md.bvh_spec().scenes())  # ico3, soup, sliver, coincident, fan
    out.update({k: md.meshes()[k] for k in ("stack", "bad")})
    return out, np.asarray(md.bvh_spec().EYE, f32)


def query_set(v, f, rows, seed):
    """points on vertices and faces, in the box and far away, rays at them from the eye and out of them, a probe-lit floor"""
    rng = np.random.default_rng(seed)
    ok = (f >= 0).all(1) & (f < len(v)).all(1)
    tri = np.nan_to_num(v[f[ok]].astype(np.float64), nan=0.0, posinf=1.0, neginf=-1.0)
    pick = tri[rng.integers(0, len(tri), rows)]
    w = rng.dirichlet([1, 1, 1], rows)
    w[::4] = np.eye(3)[rng.integers(0, 3, len(w[::4]))]  # every fourth on a vertex
    pts = (pick * w[:, :, None]).sum(1)
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    pts[1::4] = rng.uniform(lo - 0.1, hi + 0.1, pts[1::4].shape)
    pts[2::16] = 0.5 * (lo + hi) + 1e3 * rng.normal(size=pts[2::16].shape)
    pts = pts.astype(f32)
    pts[rows // 2] = [0.1, np.nan, 0.2]
    pts[rows - 2] = [np.inf, 0.0, 0.0]
    return pts, rng.normal(size=(rows, 3)).astype(f32)


def run(out_path):
    import torch
    from pano_nerf_amd import _lib
    if os.environ.get("PN_LIB"):
        _lib.LIB_PATH = os.path.abspath(os.environ["PN_LIB"])
    from pano_nerf_amd import meshdist, objects, winding
    dev = torch.device("cuda:0")
    T = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    probe = torch.rand(3, 8, 16, generator=torch.Generator().manual_seed(5)).to(dev) * 4.0
    scenes, eye = meshes()
    out = {}

    def keep(group, key, tensors):
        for i, t in enumerate(tensors if isinstance(tensors, (tuple, list)) else [tensors]):
            a = t.detach().cpu().contiguous()
            out[f"{group}|{key}|{i}"] = (a.to(torch.uint8) if a.dtype == torch.bool else a).numpy()

    for name, (v, f) in scenes.items():
        tv, tf = T(v), T(f.astype(np.int32))
        tree = objects.MeshBVH.build(tv, tf)
        keep("bvh_tree", name, tree.nodes)
        keep("bvh_moments", name, winding._moments(tree, tv, tf, dev))
        for rows in (65, 257):
            pts, dirs = query_set(v, f, rows, seed=rows)
            tp = T(pts)
            o = np.concatenate([np.broadcast_to(eye, (rows - rows // 2, 3)), pts[:rows // 2]]).astype(f32)
            d = np.concatenate([pts[:rows - rows // 2] - eye, dirs[:rows // 2]]).astype(f32)
            to, td = T(o), T(d)
            normals = T(np.broadcast_to(f32([0.0, 0.0, 1.0]), (rows, 3)))
            for tag, accel in (("brute", None), ("bvh", tree)):
                key = f"{name}|{rows}|{tag}"
                t, face, bary = objects.trace_mesh(to, td, tv, tf, accel=accel)
                keep("trace_mesh", key, (t, face, bary, objects.trace_mesh(to, td, tv, tf, any_hit=True, accel=accel)))
                tm = torch.where(torch.isfinite(t) & (torch.arange(rows, device=dev) % 2 == 0), t, 2.0 * t.clamp(max=10.0))
                keep("trace_mesh t_max", key, objects.trace_mesh(to, td, tv, tf, t_max=tm, accel=accel)
                     + (objects.trace_mesh(to, td, tv, tf, t_max=tm, any_hit=True, accel=accel),))
                keep("shadow_ratio", key, objects.shadow_ratio(tp, normals, probe, tv, tf, bias=1e-3, accel=accel))
                cp = meshdist.closest_point(tp, tv, tf, accel=accel)
                reach = float(cp[0][torch.isfinite(cp[0])].median()) if bool(torch.isfinite(cp[0]).any()) else 1.0
                keep("closest_point", key, cp + meshdist.closest_point(tp, tv, tf, max_distance=reach, accel=accel))
                for beta in (2.0, 4.0):
                    keep("winding_number", f"{key}|{beta:g}", winding.winding_number(tp, tv, tf, accel=accel, beta=beta))
                keep("signed_distance", key, winding.signed_distance(tp, tv, tf, accel=accel)
                     + winding.signed_distance(tp, tv, tf, max_distance=reach, accel=accel))
    torch.cuda.synchronize()
    np.savez(out_path, **out)
    print(f"{len(out)} outputs from {_lib.LIB_PATH} -> {out_path}")


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), "the two runs hold different outputs"
    groups = {}
    for k in a.files:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, k
        pad = (-x.nbytes) % 4
        wx, wy = (np.frombuffer(z.tobytes() + b"\0" * pad, np.uint32) for z in (x, y))
        g = groups.setdefault(k.split("|")[0], [0, 0, 0])
        g[0], g[1], g[2] = g[0] + 1, g[1] + len(wx), g[2] + int((wx != wy).sum())
    for name, (n, words, differ) in sorted(groups.items()):
        print(f"   {name:18s} {n:5d} outputs, {words:9d} 32-bit words, {differ} differ")
    bad = sum(g[2] for g in groups.values())
    print("   ALL EQUAL" if not bad else f"   {bad} WORDS DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("OLD", "NEW"))
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else run(args.out))
