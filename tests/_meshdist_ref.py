"""numpy fp64 restatement of include/panonerf_hip.h, section "mesh distance": the point / triangle distance with its
closest point and barycentrics (Ericson's regions, operation for operation), the box bound lb on the padded boxes of
test_bvh_cpu.py, the candidate rule with a count of its violations, the answer (brute force only: there is no tree here),
the sampling integers and samples, and the scores of compare_meshes.  numpy's +, -, *, / and sqrt on float64 are the IEEE
operations the kernels run with -ffp-contract=off, so the fp64 values here are the kernels' own and every fp32 output is
the same value rounded once.

Also the meshes and query points that test_meshdist_cpu.py and test_gpu_meshdist.py share."""
import functools
import importlib.util
import os

import numpy as np

f32, f64 = np.float32, np.float64
TILE = 256  # PN_MESHDIST_TILE
WEIGHT_ONE = 2147483648.0  # PN_MESHDIST_WEIGHT_ONE
R2_A1, R2_A2 = 0.7548776662466927, 0.5698402909980532  # PN_MESHDIST_R2_A1, PN_MESHDIST_R2_A2
LB_FACTOR = 1.0 - 2.0 ** -40


@functools.lru_cache(None)
def bvh_spec():
    s = importlib.util.spec_from_file_location("_bvh_spec_for_meshdist", os.path.join(os.path.dirname(__file__), "test_bvh_cpu.py"))
    m = importlib.util.module_from_spec(s)
    s.loader.exec_module(m)
    return m


# ------------------------------------------------------------------------------------------------- point / triangle
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def along(s, e, t):
    return s + e * t[..., None]


def dist2(p, q):
    r = p - q
    return dot(r, r)


def seg_t(p, s, se):
    L = dot(se, se)
    t = dot(p - s, se) / L
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    return np.where(L > 0.0, t, 0.0)


def valid_faces(vertices, faces):
    """[F] bool: every index in [0, V) and every coordinate finite; and the corners [F, 3, 3] fp64 (0 where not valid)"""
    vt, fc = np.asarray(vertices, f32), np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((fc >= 0) & (fc < len(vt))).all(1) if len(fc) else np.zeros(0, bool)
    tri = vt[np.where(ok[:, None], fc, 0)] if len(vt) else np.zeros((len(fc), 3, 3), f32)
    ok = ok & np.isfinite(tri).all((1, 2))
    return ok, np.where(ok[:, None, None], tri, 0).astype(f64)


def point_tri(p, a, b, c):
    """(d2, q, u, v) of points p against triangles a, b, c (fp64 arrays that broadcast against each other, last axis 3)"""
    with np.errstate(all="ignore"):
        shape = np.broadcast(p[..., 0], a[..., 0]).shape
        p, a, b, c = (np.broadcast_to(x, shape + (3,)) for x in (p, a, b, c))
        ab, ac = b - a, c - a
        n = cross(ab, ac)
        flat = dot(n, n) == 0.0
        # the face without area: segments ab, bc, ca
        t = seg_t(p, a, ab)
        sq, su, sv = along(a, ab, t), t, np.zeros(shape)
        sd = dist2(p, sq)
        bc = c - b
        t = seg_t(p, b, bc)
        q2 = along(b, bc, t)
        e = dist2(p, q2)
        m = e < sd
        sd, sq, su, sv = np.where(m, e, sd), np.where(m[..., None], q2, sq), np.where(m, 1.0 - t, su), np.where(m, t, sv)
        ca = a - c
        t = seg_t(p, c, ca)
        q2 = along(c, ca, t)
        e = dist2(p, q2)
        m = e < sd
        sd, sq, su, sv = np.where(m, e, sd), np.where(m[..., None], q2, sq), np.where(m, 0.0, su), np.where(m, 1.0 - t, sv)
        # the regions, the first that holds
        ap = p - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        g, h = d4 - d3, d5 - d6
        one, zero = np.ones(shape), np.zeros(shape)
        tab, tac, tbc = d1 / (d1 - d3), d2 / (d2 - d6), g / (g + h)
        den = 1.0 / ((va + vb) + vc)
        ui, vi = vb * den, vc * den
        rules = [  # (condition, q, u, v)
            ((d1 <= 0.0) & (d2 <= 0.0), a, zero, zero),
            ((d3 >= 0.0) & (d4 <= d3), b, one, zero),
            ((vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), along(a, ab, tab), tab, zero),
            ((d6 >= 0.0) & (d5 <= d6), c, zero, one),
            ((vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), along(a, ac, tac), zero, tac),
            ((va <= 0.0) & (g >= 0.0) & (h >= 0.0), along(b, c - b, tbc), 1.0 - tbc, tbc),
        ]
        q, u, v = along(along(a, ab, ui), ac, vi), ui, vi  # the interior
        for cond, rq, ru, rv in reversed(rules):
            q, u, v = np.where(cond[..., None], rq, q), np.where(cond, ru, u), np.where(cond, rv, v)
        q, u, v = np.where(flat[..., None], sq, q), np.where(flat, su, u), np.where(flat, sv, v)
        d = np.where(flat, sd, dist2(p, q))
    return d, q, u, v


def box_lb(p, lo, hi):
    """lb [P, B] of points p [P, 3] (fp64) against fp32 boxes lo, hi [B, 3]; +inf for an empty box"""
    with np.errstate(all="ignore"):
        lo, hi = np.asarray(lo, f32).astype(f64)[None], np.asarray(hi, f32).astype(f64)[None]
        pp = p[:, None, :]
        g = np.maximum(np.maximum(lo - pp, 0.0), pp - hi)
        lb = ((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]) * LB_FACTOR
        return np.where(lo[..., 0] <= hi[..., 0], lb, np.inf)


def closest_point(points, vertices, faces, max_distance=None, chunk=64):
    """The contract's answer for every point, brute force over the candidates: a dict with distance [P] fp32, face [P]
    int32, closest [P, 3] fp32, bary [P, 2] fp32, the fp64 values behind them (d2, q, uv), `violations` = the (finite point,
    valid face) pairs that fail the candidate rule lb <= d2, and `margin` = the smallest d2 - lb over the pairs whose point
    lies outside the face's padded box (lb > 0)."""
    pts = np.asarray(points, f32)
    P = len(pts)
    out = dict(distance=np.full(P, np.inf, f32), face=np.full(P, -1, np.int32), closest=np.zeros((P, 3), f32),
               bary=np.zeros((P, 2), f32), d2=np.full(P, np.inf), q=np.zeros((P, 3)), uv=np.zeros((P, 2)), violations=0,
               margin=np.inf)
    ok, tri = valid_faces(vertices, faces)
    if not ok.any():
        return out
    best0 = np.inf if max_distance is None else f64(f32(max_distance)) * f64(f32(max_distance))
    lo, hi = bvh_spec().tri_boxes(vertices, faces)
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    for first in range(0, P, chunk):
        sl = slice(first, min(first + chunk, P))
        p = pts[sl].astype(f64)
        fin = np.isfinite(p).all(1)
        p = np.where(fin[:, None], p, 0.0)
        d, q, u, v = point_tri(p[:, None, :], a, b, c)
        lb = box_lb(p, lo, hi)
        pair = fin[:, None] & ok[None, :]
        cand = pair & (lb <= d)
        out["violations"] += int((pair & ~cand).sum())
        outside = pair & (lb > 0.0)
        if outside.any():
            out["margin"] = min(out["margin"], float((d - lb)[outside].min()))
        dc = np.where(cand, d, np.inf)
        j = np.argmin(dc, 1)  # the first minimum: the lowest face index among equal d2
        r = np.arange(len(p))
        found = cand[r, j] & (dc[r, j] <= best0)
        idx = np.arange(first, first + len(p))[found]
        jj, rr = j[found], r[found]
        out["d2"][idx], out["q"][idx], out["uv"][idx] = d[rr, jj], q[rr, jj], np.stack([u[rr, jj], v[rr, jj]], -1)
        out["face"][idx] = jj
    hit = out["face"] >= 0
    out["distance"][hit] = np.sqrt(out["d2"][hit]).astype(f32)
    out["closest"][hit], out["bary"][hit] = out["q"][hit].astype(f32), out["uv"][hit].astype(f32)
    return out


# ------------------------------------------------------------------------------------------------------------ sampling
def face_weights(vertices, faces):
    """(area [F] fp64, weight [F] int64, cum [F] int64)"""
    ok, tri = valid_faces(vertices, faces)
    n = cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = np.where(ok, 0.5 * np.sqrt(dot(n, n)), 0.0)
    m = area.max() if len(area) else 0.0
    with np.errstate(all="ignore"):
        w = np.where((m > 0.0) & np.isfinite(m) & (area > 0.0), np.floor(area / m * WEIGHT_ONE), 0.0).astype(np.int64)
    return area, w, np.cumsum(w)


def thresholds(W, count):
    i = np.arange(count, dtype=np.int64)
    return i * (W // count) + i * (W % count) // count


def sample_surface(vertices, faces, count):
    """dict: face [count] int32, points [count, 3] and bary [count, 2] as fp64 (before the one rounding) and fp32, weight, W"""
    ok, tri = valid_faces(vertices, faces)
    area, w, cum = face_weights(vertices, faces)
    W = int(cum[-1]) if len(cum) else 0
    if W <= 0:
        raise ValueError("no face with area")
    t = thresholds(W, count)
    f = np.searchsorted(cum, t, side="right")  # the first face whose running weight exceeds t
    i = np.arange(count, dtype=np.int64).astype(f64)
    x1, x2 = 0.5 + R2_A1 * i, 0.5 + R2_A2 * i
    r1, r2 = x1 - np.floor(x1), x2 - np.floor(x2)
    fold = r1 + r2 > 1.0
    r1, r2 = np.where(fold, 1.0 - r1, r1), np.where(fold, 1.0 - r2, r2)
    a, b, c = tri[f, 0], tri[f, 1], tri[f, 2]
    q = along(along(a, b - a, r1), c - a, r2)
    uv = np.stack([r1, r2], -1)
    return dict(face=f.astype(np.int32), q=q, uv=uv, points=q.astype(f32), bary=uv.astype(f32), weight=w, W=W, thresholds=t)


def face_normals(vertices, faces, idx):
    tri = np.asarray(vertices, f32)[np.asarray(faces, np.int64)[idx]].astype(f64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)


def compare_meshes(a, b, samples, taus):
    """the scores of meshdist.compare_meshes from this file's samples and brute-force answers, sums in fp64; also the
    terms, for the summation bound"""
    (va, fa), (vb, fb) = a, b
    sa, sb = sample_surface(va, fa, samples), sample_surface(vb, fb, samples)
    ab, ba = closest_point(sa["points"], vb, fb), closest_point(sb["points"], va, fa)
    dab, dba = ab["distance"].astype(f64), ba["distance"].astype(f64)
    nab = np.abs((face_normals(va, fa, sa["face"]) * face_normals(vb, fb, ab["face"])).sum(1))
    nba = np.abs((face_normals(vb, fb, sb["face"]) * face_normals(va, fa, ba["face"])).sum(1))
    n = samples
    acc, comp = dab.sum() / n, dba.sum() / n
    p = tuple(float((dab <= t).sum()) / n for t in taus)
    r = tuple(float((dba <= t).sum()) / n for t in taus)
    return {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "rms_ab": np.sqrt((dab * dab).sum() / n),
            "rms_ba": np.sqrt((dba * dba).sum() / n), "hausdorff_ab": dab.max(), "hausdorff_ba": dba.max(),
            "hausdorff": max(dab.max(), dba.max()), "precision": p, "recall": r,
            "fscore": tuple(2 * x * y / (x + y) if x + y > 0 else 0.0 for x, y in zip(p, r)),
            "normal_consistency": (nab.sum() + nba.sum()) / (2 * n), "dab": dab, "dba": dba}


# ------------------------------------------------------------------------------------------------- meshes and points
def cube():
    """the unit cube [0, 1]^3, 12 faces wound outwards; faces 0, 1 are z = 0, 2, 3 are z = 1"""
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], f32)
    f = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                  [1, 3, 5], [3, 7, 5]], np.int32)
    return v, f


def quads(h, n=4):
    """two parallel squares [0, 1]^2 at z = 0 and z = h with the same footprint, n x n cells of two triangles each, cut along
    different diagonals: (a, b)"""
    g = np.linspace(0.0, 1.0, n + 1)
    x, y = np.meshgrid(g, g, indexing="ij")
    idx = np.arange((n + 1) ** 2).reshape(n + 1, n + 1)
    p00, p10, p01, p11 = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    fa = np.concatenate([np.stack([p00, p10, p11], 1), np.stack([p00, p11, p01], 1)]).astype(np.int32)
    fb = np.concatenate([np.stack([p00, p10, p01], 1), np.stack([p10, p11, p01], 1)]).astype(np.int32)
    va = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], 1).astype(f32)
    vb = va.copy()
    vb[:, 2] = h
    return (va, fa), (vb, fb)


@functools.lru_cache(None)
def meshes():
    """name -> (vertices fp32, faces int32): the meshes of the issue's list"""
    s = bvh_spec()
    iv, ifc = s.spec.icosphere(3, s.RADIUS, s.CENTRE)
    out = {f"ico3[:{k}]": (iv, ifc[:k].copy()) for k in (1, 2, 3, TILE - 1, TILE, TILE + 1)}
    out["ico3"] = (iv, ifc)
    out["cube"] = cube()
    rng = np.random.default_rng(2)  # test_gpu_bvh.py's "stack": 4096 triangles (p, -p, 0), every box centre exactly 0, one
    F = 4096  # Morton key; each is a face without area (three collinear corners): the segment branch
    off = (rng.normal(size=(F, 3)) * 0.1).astype(f32)
    out["stack"] = (np.concatenate([off, -off, np.zeros((F, 3), f32)]),
                    np.stack([np.arange(F), np.arange(F) + F, np.arange(F) + 2 * F], 1).astype(np.int32))
    bv, bf = iv.copy(), ifc.copy()  # faces that index outside the vertices, and a vertex that is not finite
    bf[::3, 1] = len(bv) + 7
    bf[5, 0] = -1
    bv[17, 1] = np.nan
    bv[40, 0] = np.inf
    out["bad"] = (bv, bf)
    ang = np.concatenate([np.linspace(0, 2 * np.pi, 9)[:-1], 0.3 + 2e-6 * np.arange(64)])  # 8 wide blades, then slivers a few
    rim = s.CENTRE + 0.3 * np.stack([np.cos(ang), np.sin(ang), 0.2 * np.cos(3 * ang)], 1)  # fp32 ulp wide (some collapse)
    fv = np.concatenate([s.CENTRE[None] + [[0, 0, 0.05]], rim])
    ff = [[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)] + [[0, 9 + k, 10 + k] for k in range(63)]
    ff += [[0, 9, 9], [3, 3, 3]]  # repeated indices: a segment and a point
    out["sliver fan"] = (fv.astype(f32), np.array(ff, np.int32))
    return out


@functools.lru_cache(None)
def query_points(name):
    """1000 fp32 points for mesh `name` (not a multiple of 64): on vertices, on edge midpoints and on faces (as fp32 sees
    them), inside the mesh's box, 10^3 mesh sizes away, a NaN row and an inf row"""
    v, f = meshes()[name]
    ok, tri = valid_faces(v, f)
    tri = tri[ok]
    rng = np.random.default_rng(7)
    corners = tri.reshape(-1, 3)
    lo, hi = corners.min(0), corners.max(0)
    size = max(float((hi - lo).max()), 1e-3)
    pick = lambda n: tri[rng.integers(0, len(tri), n)]
    t = pick(150)
    on_v = t[np.arange(150), rng.integers(0, 3, 150)]
    t = pick(150)
    k = rng.integers(0, 3, 150)
    on_e = 0.5 * (t[np.arange(150), k] + t[np.arange(150), (k + 1) % 3])
    w = rng.dirichlet([1, 1, 1], 200)
    on_f = (pick(200) * w[:, :, None]).sum(1)
    box = rng.uniform(lo - 0.1 * size, hi + 0.1 * size, (300, 3))
    d = rng.normal(size=(198, 3))
    far = 0.5 * (lo + hi) + 1e3 * size * d / np.linalg.norm(d, axis=1, keepdims=True)
    pts = np.concatenate([on_v, on_e, on_f, box, far, np.zeros((2, 3))]).astype(f32)
    pts[998] = [0.1, np.nan, 0.2]
    pts[999] = [np.inf, 0.0, 0.0]
    assert len(pts) == 1000 and len(pts) % 64
    return pts


@functools.lru_cache(None)
def answer(name, max_distance=None):
    v, f = meshes()[name]
    return closest_point(query_points(name), v, f, max_distance)
