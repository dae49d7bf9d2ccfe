"""numpy restatement of the mesh operations of include/panonerf_hip.h ("mesh operations"): components by a plain flood fill,
the component records and the quadric vertex clustering operation for operation in fp64 on fp32 inputs, in the orders the
header states, so that +, -, *, / and sqrt (all correctly rounded, the library builds with -ffp-contract=off) give the same
bits.  Also the small meshes the CPU and GPU tests share.

Fragile clusters: the only discrete decisions of the solve are `t == 0` and `|x_k| <= cell / 2`; a cluster is marked
fragile when | |x_k| - cell / 2 | <= 1e-9 cell for some k, or when t is non-zero but below 1e-300.  The cell index is not
fragile: it is one correctly rounded fp64 division and a floor on both sides."""
import collections

import numpy as np

F64 = np.float64
NO_FACE = np.iinfo(np.int64).max


def f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------- meshes
def grid_plane(n=64, tilt=(0.5, 0.25)):
    """(n + 1)^2 vertices on z = tilt_x x + tilt_y y over [0, 2]^2, every coordinate a dyadic rational (exact in fp32)"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    x, y = i * (2.0 / n), j * (2.0 / n)
    v = np.stack([x, y, tilt[0] * x + tilt[1] * y], -1).reshape(-1, 3)
    idx = lambda a, b: a * (n + 1) + b
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    f = np.concatenate([np.stack([idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)], 1),
                        np.stack([idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)], 1)])
    return f32(v), f.astype(np.int32)


def weld(v, f):
    """merge vertices at identical positions (first occurrence order), drop nothing else"""
    _, first, inv = np.unique(np.round(v * 4096).astype(np.int64), axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)
    new = np.empty_like(order)
    new[order] = np.arange(len(order))
    return v[first[order]], new[inv.reshape(-1)][f].astype(np.int32)


def cube(n=16):
    """the closed surface of [-1, 1]^3, n x n quads per side, welded, wound outwards"""
    vs, fs = [], []
    t = np.linspace(-1.0, 1.0, n + 1)
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    idx = lambda p, q: p * (n + 1) + q
    quads = np.concatenate([np.stack([idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)], 1),
                            np.stack([idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)], 1)])
    U, W = np.meshgrid(t, t, indexing="ij")
    for axis in range(3):
        for sign in (-1.0, 1.0):
            p = np.empty((n + 1, n + 1, 3))
            p[..., axis] = sign
            p[..., (axis + 1) % 3] = U
            p[..., (axis + 2) % 3] = W
            q = quads if sign > 0 else quads[:, ::-1]
            fs.append(q + sum(len(x) for x in vs))
            vs.append(p.reshape(-1, 3))
    v, f = weld(np.concatenate(vs), np.concatenate(fs))
    return f32(v), f


def icosphere(level=4, radius=1.0, centre=(0.0, 0.0, 0.0)):
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, F64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return f32(np.asarray(v) * radius + np.asarray(centre, F64)), np.asarray(f, np.int32)


def join(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def permuted(v, f, seed):
    """the same mesh with its vertex indices randomly permuted (long union-find chains) and its faces shuffled"""
    rng = np.random.RandomState(seed)
    p = rng.permutation(len(v))  # new index of old vertex i
    nv = np.empty_like(v)
    nv[p] = v
    nf = p[f].astype(np.int32)
    return nv, nf[rng.permutation(len(nf))]


def strip(n=4096):
    """n triangles in a row over two rails of vertices"""
    k = n // 2 + 1
    x = np.arange(k, dtype=F64) * 0.125
    v = np.concatenate([np.stack([x, 0 * x, 0.25 * x], 1), np.stack([x, 1 + 0 * x, 0.5 * x], 1)])
    i = np.arange(k - 1)
    f = np.concatenate([np.stack([i, i + 1, k + i], 1), np.stack([i + 1, k + i + 1, k + i], 1)])
    return f32(v), f.astype(np.int32)


def serpentine(rows=24, cols=40):
    """a band that runs to and fro: rows of quads joined at alternating ends only"""
    vs, fs, off = [], [], 0
    for r in range(rows):
        x = np.arange(cols + 1, dtype=F64) * 0.25
        lo = np.stack([x, np.full_like(x, 2.0 * r), 0.125 * x], 1)
        hi = np.stack([x, np.full_like(x, 2.0 * r + 1.0), 0.125 * x], 1)
        vs += [lo, hi]
        i = np.arange(cols)
        k = cols + 1
        fs.append(np.concatenate([np.stack([i, i + 1, k + i], 1), np.stack([i + 1, k + i + 1, k + i], 1)]) + off)
        if r:  # one bridge triangle pair to the row below, at the right or left end in turn
            e = cols if r % 2 else 0
            below_hi, this_lo = off - (cols + 1) + e, off + e
            nb = e - 1 if e else 1
            fs.append(np.asarray([[below_hi, this_lo, off - (cols + 1) + nb]]))
        off += 2 * (cols + 1)
    return f32(np.concatenate(vs)), np.concatenate(fs).astype(np.int32)


def fans():
    """two fans of 6 triangles that touch in ONE shared vertex index (vertex 0): one component"""
    ang = np.linspace(0.0, np.pi / 2, 7)
    a = np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)
    b = np.stack([-np.cos(ang), -np.sin(ang), 0.5 + 0 * ang], 1)
    v = np.concatenate([[[0.0, 0.0, 0.0]], a, b])
    f = [(0, 1 + i, 2 + i) for i in range(6)] + [(0, 8 + i, 9 + i) for i in range(6)]
    return f32(v), np.asarray(f, np.int32)


def floater():
    """a 4-face tetrahedron far from everything"""
    v = np.asarray([[5, 5, 5], [5.25, 5, 5], [5, 5.25, 5], [5, 5, 5.25]], F64)
    return f32(v), np.asarray([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.int32)


def component_cases():
    """name -> (vertices, faces): every components case of the tests"""
    two = join(icosphere(2, 1.0), icosphere(1, 0.5, (3.0, 0.25, 0.0)), floater())
    lone = join(fans(), (f32([[9, 9, 9], [8, 8, 8]]), np.zeros((0, 3), np.int32)))  # two unreferenced vertices at the end
    v, f = lone
    lone = (np.concatenate([f32([[7, 7, 7]]), v]), f + 1)  # and one at the start
    return collections.OrderedDict([
        ("spheres_floater", two), ("fans", fans()), ("strip", permuted(*strip(4096), seed=1)),
        ("strip_long", permuted(*strip(9000), seed=3)),  # three chunks of the records' two-level sum, the last one partial
        ("serpentine", permuted(*serpentine(), seed=2)), ("unreferenced", lone),
        ("triangle", (f32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.asarray([[0, 1, 2]], np.int32))),
        ("empty", (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)))])


SIMPLIFY_CASES = [("plane", 0.3), ("cube", 0.25), ("cube", 0.3), ("cube", 0.5), ("ico", 0.25), ("ico", 0.3), ("ico", 0.5)]


def simplify_case(name):
    """(vertices, faces, origin): the cube and the icosphere with the grid origin 0.01 below the vertex minimum (with the
    default origin every vertex of the cube's far sides would sit exactly on a cell wall, a fragile decision by design)"""
    v, f = {"plane": grid_plane, "cube": cube, "ico": icosphere}[name]()
    return v, f, (None if name == "plane" else f32(v.min(0).astype(F64) - 0.01))


def attributes(v, seed=5):
    """per-vertex normals (unit) and colours for the averaging tests"""
    rng = np.random.RandomState(seed)
    n = rng.standard_normal(v.shape)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return f32(n), f32(rng.uniform(0, 1, v.shape))


# ------------------------------------------------------------------------------------------------------ components
def components(faces, V):
    """(vertex_label [V], face_label [F], count) by a plain flood fill over the vertex adjacency, components numbered in
    ascending order of their smallest vertex index, -1 for a vertex no face uses"""
    faces = np.asarray(faces, np.int64)
    adj = [[] for _ in range(V)]
    for a, b, c in faces:
        adj[a] += [b, c]
        adj[b] += [a, c]
        adj[c] += [a, b]
    used = np.zeros(V, bool)
    used[faces.reshape(-1)] = True
    vlab = np.full(V, -1, np.int32)
    count = 0
    for s in range(V):  # ascending: the seed is the smallest index of its component
        if not used[s] or vlab[s] >= 0:
            continue
        vlab[s] = count
        stack = [s]
        while stack:
            p = stack.pop()
            for q in adj[p]:
                if vlab[q] < 0:
                    vlab[q] = count
                    stack.append(q)
        count += 1
    flab = vlab[faces[:, 0]].astype(np.int32) if len(faces) else np.zeros(0, np.int32)
    return vlab, flab, count


def _chunk_sum(x):
    """one workgroup's sum of a chunk x (at most 4096): thread t adds t, t + 256, ... in order from 0.0, xor butterfly 32 .. 1
    within a wave, then waves 0, 1, 2, 3 in order"""
    n = len(x)
    it = -(-n // 256)
    pad = np.zeros(it * 256, F64)
    pad[:n] = x
    acc = np.zeros(256, F64)
    for row in pad.reshape(it, 256):
        acc = acc + row
    lanes = acc.reshape(4, 64)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ o]
    w = lanes[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def _tree_sum(x):
    """the sum of a component's list: chunks of 4096 by _chunk_sum, then the chunks in order, sequentially, from 0.0"""
    total = F64(0.0)
    for j in range(0, len(x), 4096):
        total = total + _chunk_sum(x[j:j + 4096])
    return total


def component_stats(v, f, flab, vlab, C):
    v64 = np.asarray(v, np.float32).astype(F64)
    out = dict(faces=np.zeros(C, np.int32), vertices=np.zeros(C, np.int32), area=np.zeros(C, F64), volume=np.zeros(C, F64),
               bbox=np.zeros((C, 6), np.float32))
    for c in range(C):
        fc = f[flab == c].astype(np.int64)  # ascending face index
        a, b, d = v64[fc[:, 0]], v64[fc[:, 1]], v64[fc[:, 2]]
        u, w = b - a, d - a
        n0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        n1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        n2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        x0 = b[:, 1] * d[:, 2] - b[:, 2] * d[:, 1]
        x1 = b[:, 2] * d[:, 0] - b[:, 0] * d[:, 2]
        x2 = b[:, 0] * d[:, 1] - b[:, 1] * d[:, 0]
        out["area"][c] = _tree_sum(np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)) / 2.0
        out["volume"][c] = _tree_sum((a[:, 0] * x0 + a[:, 1] * x1) + a[:, 2] * x2) / 6.0
        out["faces"][c] = len(fc)
        out["vertices"][c] = int((vlab == c).sum())
        pts = np.asarray(v, np.float32)[fc.reshape(-1)]
        out["bbox"][c] = np.concatenate([pts.min(0), pts.max(0)])
    return out


def compact(v, f, keep_face, normals=None, colors=None):
    face_map = np.nonzero(keep_face)[0].astype(np.int32)
    kept = f[face_map]
    used = np.zeros(len(v), bool)
    used[kept.reshape(-1)] = True
    vertex_map = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    g = lambda t: None if t is None else t[used]
    return (v[used], vertex_map[kept].astype(np.int32).reshape(-1, 3), g(normals), g(colors)), vertex_map, face_map


def filter_components(v, f, min_faces=0, min_area=0.0, keep_largest=None, by="area", normals=None, colors=None):
    V = len(v)
    if len(f) == 0:
        return (v[:0], f, None, None), np.full(V, -1, np.int32), np.zeros(0, np.int32)
    vlab, flab, C = components(f, V)
    st = component_stats(v, f, flab, vlab, C)
    area32 = st["area"].astype(np.float32)
    keep = (st["faces"] >= min_faces) & (area32 >= np.float32(min_area))
    if keep_largest is not None:
        size = {"area": area32, "faces": st["faces"].astype(np.float32), "vertices": st["vertices"].astype(np.float32),
                "volume": np.abs(st["volume"].astype(np.float32))}[by]
        size = np.where(keep, size, np.float32(-1.0))
        order = np.argsort(-size, kind="stable")
        top = np.zeros(C, bool)
        top[order[:keep_largest]] = True
        keep &= top
    return compact(v, f, keep[flab], normals, colors)


# ------------------------------------------------------------------------------------------------------ clustering
def cells(v, cell, origin=None):
    """(lo fp32 [3], cell as an fp32 value, n [3]) as meshops._cells"""
    c = float(np.float32(cell))
    lo = v.min(0).astype(np.float32) if origin is None else f32(origin)
    n = [int(max(np.floor((F64(v[:, a].max()) - F64(lo[a])) / c), 0)) + 1 for a in range(3)]
    return lo, c, n


def cluster_keys(v, lo, cell, n):
    q = np.floor((v.astype(F64) - lo.astype(F64)) / F64(cell))
    q = np.clip(q, 0, np.asarray(n, F64) - 1).astype(np.int64)
    return (q[:, 0] * n[1] + q[:, 1]) * n[2] + q[:, 2]


def _seq_sum(values, starts):
    """per segment the sequential sum, from 0.0, of its rows in order: values [N, d] grouped, starts [K + 1]"""
    cnt = np.diff(starts)
    acc = np.zeros((len(cnt), values.shape[1]), F64)
    for j in range(int(cnt.max()) if len(cnt) else 0):
        m = cnt > j
        acc[m] = acc[m] + values[starts[:-1][m] + j]
    return acc


def cluster_faces(f, rank):
    rf = rank[f.astype(np.int64)].astype(np.int32).reshape(-1, 3)
    s = np.sort(rf.astype(np.int64), axis=1)
    key = (s[:, 0] << 42) | (s[:, 1] << 21) | s[:, 2]
    dead = (rf[:, 0] == rf[:, 1]) | (rf[:, 1] == rf[:, 2]) | (rf[:, 0] == rf[:, 2])
    key = np.where(dead, NO_FACE, key)
    keep = np.zeros(len(f), bool)
    live = np.nonzero(~dead)[0]
    _, first = np.unique(key[live], return_index=True)  # the first occurrence = the lowest face index
    keep[live[first]] = True
    return rf, key, keep


def simplify(v, f, cell, origin=None, lam=1e-3, normals=None, colors=None, order=None):
    """Everything simplify_mesh returns and the intermediates, as a dict.  `order`: None follows the header's order; a
    numpy RandomState permutes the summation order within every cluster (the order-independence test)."""
    v = np.asarray(v, np.float32)
    V, F = len(v), len(f)
    lo, c, n = cells(v, cell, origin)
    keys = cluster_keys(v, lo, c, n)
    ckeys, rank = np.unique(keys, return_inverse=True)
    rank = rank.reshape(-1).astype(np.int32)
    K = len(ckeys)
    rf, fkey, keep = cluster_faces(f, rank)
    iz, iy, ix = ckeys % n[2], (ckeys // n[2]) % n[1], ckeys // (n[2] * n[1])
    cen = lo.astype(F64)[None] + (np.stack([ix, iy, iz], 1).astype(F64) + 0.5) * F64(c)

    def grouped(group_of, count):
        o = np.argsort(group_of, kind="stable")
        st = np.searchsorted(group_of[o], np.arange(count + 1))
        if order is not None:
            o = o.copy()
            for k in range(count):
                o[st[k]:st[k + 1]] = order.permutation(o[st[k]:st[k + 1]])
        return o, st

    vo, vs = grouped(rank, K)
    cnt = np.diff(vs).astype(F64)[:, None]
    v64 = v.astype(F64)
    xbar = _seq_sum(v64[vo] - cen[rank[vo]], vs) / cnt
    out_n = out_c = None
    if normals is not None:
        g = _seq_sum(np.asarray(normals, np.float32).astype(F64)[vo], vs) / cnt
        nn = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = nn >= 1e-12
        out_n = np.where(ok[:, None], g / np.where(ok, nn, 1.0)[:, None], 0.0)
    if colors is not None:
        out_c = _seq_sum(np.asarray(colors, np.float32).astype(F64)[vo], vs) / cnt

    inc = rank[f.astype(np.int64).reshape(-1)] if F else np.zeros(0, np.int32)
    io, ist = grouped(inc, K)
    ff = f.astype(np.int64)[io // 3] if F else np.zeros((0, 3), np.int64)
    a, b, d = v64[ff[:, 0]], v64[ff[:, 1]], v64[ff[:, 2]]
    u, w = b - a, d - a
    n0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    n1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    n2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    p = a - cen[inc[io]]
    dd = -((n0 * p[:, 0] + n1 * p[:, 1]) + n2 * p[:, 2])
    q = _seq_sum(np.stack([n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2, n0 * dd, n1 * dd, n2 * dd], 1), ist)
    A00, A01, A02, A11, A12, A22, b0, b1, b2 = q.T
    t = (A00 + A11) + A22
    with np.errstate(all="ignore"):
        sh = lam * t
        q00, q11, q22 = A00 + sh, A11 + sh, A22 + sh
        r0, r1, r2 = sh * xbar[:, 0] - b0, sh * xbar[:, 1] - b1, sh * xbar[:, 2] - b2
        l10, l20 = A01 / q00, A02 / q00
        d1 = q11 - l10 * A01
        u12 = A12 - l20 * A01
        l21 = u12 / d1
        d2 = (q22 - l20 * A02) - l21 * u12
        y1 = r1 - l10 * r0
        y2 = (r2 - l20 * r0) - l21 * y1
        z2 = y2 / d2
        z1 = y1 / d1 - l21 * z2
        z0 = (r0 / q00 - l10 * z1) - l20 * z2
        z = np.stack([z0, z1, z2], 1)
        half = F64(c) * 0.5
        ok = np.isfinite(z).all(1) & (np.abs(z) <= half).all(1)
        margin = np.where(np.isfinite(z), np.abs(np.abs(z) - half), np.inf).min(1)
    solved = t != 0.0
    flags = np.where(solved, np.where(ok, 0, 1), 2).astype(np.uint8)
    x = np.where((solved & ok)[:, None], z, xbar)
    fragile = (solved & (margin <= 1e-9 * c)) | (solved & (np.abs(t) < 1e-300))
    pos = cen + x

    face_map = np.nonzero(keep)[0].astype(np.int32)
    kept = rf[face_map].astype(np.int64)
    used = np.zeros(K, bool)
    used[kept.reshape(-1)] = True
    new = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    g = lambda t_: None if t_ is None else t_[used]
    return dict(lo=lo, cell=c, n=n, keys=keys, cluster_keys=ckeys, rank=rank, K=K, centres=cen, xbar=xbar,
                A=np.stack([A00, A01, A02, A11, A12, A22], 1), b=np.stack([b0, b1, b2], 1), t=t, x=x, z=z, margin=margin,
                used=used, vertices=pos[used], faces=new[kept].astype(np.int32).reshape(-1, 3), normals=g(out_n), colors=g(out_c),
                vertex_map=new[rank], face_map=face_map, flags=flags[used], flags_all=flags, fragile=fragile[used],
                fragile_all=fragile, duplicates=int((~keep & (fkey != NO_FACE)).sum()))


def edge_counts(f):
    f = np.asarray(f, np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    ok = a != b
    a, b = a[ok], b[ok]
    if len(a) == 0:
        return {"boundary": 0, "nonmanifold": 0, "inconsistent": 0}
    base = int(max(a.max(), b.max())) + 1
    cu = np.unique(np.minimum(a, b) * base + np.maximum(a, b), return_counts=True)[1]
    cd = np.unique(a * base + b, return_counts=True)[1]
    return {"boundary": int((cu == 1).sum()), "nonmanifold": int((cu > 2).sum()), "inconsistent": int((cd > 1).sum())}


def euler(v_count, f):
    f = np.asarray(f, np.int64)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    return v_count - len(e) + len(f)
