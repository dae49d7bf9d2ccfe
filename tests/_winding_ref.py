"""numpy fp64 restatement of include/panonerf_hip.h, section "winding number": the solid angle of van Oosterom and Strackee
operation for operation, the exact sum in ascending face order, the dipole moments of every internal node of a node buffer
(test_bvh_cpu.py's host-built tree, or the device's own rows), and the pre-order Barnes-Hut walk with its visit count.
numpy's +, -, *, / and sqrt on float64 are the IEEE operations the kernels run with -ffp-contract=off, so the moments here
are the kernels' bit for bit; arctan2 is the one operation whose last bits the two libraries may round differently.

Also the meshes, the query points and the recorded error table that test_winding_cpu.py and test_gpu_winding.py share.
dot, cross, valid_faces, the cube and the icosphere are _meshdist_ref.py's."""
import functools

import numpy as np

import _meshdist_ref as md

f32, f64 = np.float32, np.float64
TILE = 256  # PN_WINDING_TILE
FOUR_PI = 12.566370614359172  # PN_WINDING_FOUR_PI
MAX_DEPTH = 94  # PN_BVH_MAX_DEPTH
dot, cross, valid_faces, bvh_spec = md.dot, md.cross, md.valid_faces, md.bvh_spec

# E(beta) = max |w_walk - w_exact| over scenes() and query_points(), as test_winding_cpu.py measured it on the host-built
# Morton tree (it prints the table and holds a fresh measurement to <= 2 x these figures); DESIGN.md 6n has the same table
RECORDED_E = {2.0: 3.69e-2, 4.0: 6.71e-3, 8.0: 1.39e-3}


# --------------------------------------------------------------------------------------------------------- solid angle
def solid_angle(p, a, b, c):
    """Omega of points p against triangles a, b, c (fp64 arrays that broadcast, last axis 3); 0 where num == 0"""
    with np.errstate(all="ignore"):
        A, B, C = a - p, b - p, c - p
        num = dot(A, cross(B, C))
        la, lb, lc = np.sqrt(dot(A, A)), np.sqrt(dot(B, B)), np.sqrt(dot(C, C))
        den = ((la * lb) * lc + dot(A, B) * lc) + (dot(B, C) * la + dot(C, A) * lb)
        return np.where(num == 0.0, 0.0, 2.0 * np.arctan2(num, den))


def _finish(S, fin):
    return np.where(fin, S / FOUR_PI, np.nan).astype(f32)


def exact(points, vertices, faces, chunk=256):
    """The brute-force contract: dict with w [P] fp32 and S [P] fp64, the terms of the valid faces summed in ascending face
    index (np.cumsum runs in order); NaN for a point that is not finite"""
    pts = np.asarray(points, f32).astype(f64).reshape(-1, 3)
    fin = np.isfinite(pts).all(1)
    p = np.where(fin[:, None], pts, 0.0)
    ok, tri = valid_faces(vertices, faces)
    S = np.zeros(len(p))
    for first in range(0, len(p), chunk):
        q = p[first:first + chunk, None, :]
        t = np.where(ok[None, :], solid_angle(q, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]), 0.0)
        if t.shape[1]:
            S[first:first + chunk] = np.cumsum(t, 1)[:, -1]
    return dict(w=_finish(S, fin), S=S)


# ------------------------------------------------------------------------------------------------------------- moments
def _refs(nodes):
    n = np.ascontiguousarray(nodes, f32).view(np.int32)
    return n[:, 3].astype(np.int64), n[:, 7].astype(np.int64), n[:, 11].astype(np.int64)


def leaf_parts(vertices, faces):
    """(g [F, 3], N [F, 3], A [F]) a leaf hands up: zeros for a face that is not valid"""
    ok, tri = valid_faces(vertices, faces)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    N = 0.5 * cross(b - a, c - a)
    A = np.sqrt(dot(N, N))
    g = ((a + b) + c) / 3.0
    z = ok[:, None]
    return np.where(z, g, 0.0), np.where(z, N, 0.0), np.where(ok, A, 0.0)


def moments(nodes, vertices, faces):
    """[max(F - 1, 1), 8] fp64 = (g, r2, N, A) of every internal node reachable from row 0 of a node buffer that is a tree
    (rows that are not reachable stay zero); children before parents, left with right in that order"""
    nodes = np.ascontiguousarray(nodes, f32)
    F = len(faces)
    out = np.zeros((max(F - 1, 1), 8))
    if F <= 1:
        return out
    left, right, _ = _refs(nodes)
    lg, lN, lA = leaf_parts(vertices, faces)

    def part(ref):
        if ref < 0:
            f = ~ref
            return (lg[f], lN[f], lA[f]) if f < F else (np.zeros(3), np.zeros(3), 0.0)
        return out[ref, 0:3], out[ref, 4:7], out[ref, 7]

    order, todo = [], [0]
    while todo:  # parents before children; reversed below
        i = todo.pop()
        order.append(i)
        todo += [int(r) for r in (left[i], right[i]) if 0 <= r < F - 1]
    for i in reversed(order):
        (gl, Nl, Al), (gr, Nr, Ar) = part(int(left[i])), part(int(right[i]))
        lo = np.minimum(nodes[i, 0:3], nodes[i, 8:11]).astype(f64)
        hi = np.maximum(nodes[i, 4:7], nodes[i, 12:15]).astype(f64)
        if not lo[0] <= hi[0]:
            continue  # the empty box: a zero row
        N, A = Nl + Nr, Al + Ar
        g = (Al * gl + Ar * gr) / A if A > 0.0 else (lo + hi) * 0.5
        e = np.maximum(g - lo, hi - g)
        out[i] = [g[0], g[1], g[2], (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], N[0], N[1], N[2], A]
    return out


# ---------------------------------------------------------------------------------------------------------------- walk
def walk(points, vertices, faces, nodes, mom, beta):
    """The walk's contract for every point, all points in lockstep (each keeps its own stack and its own order of
    summation): dict with w [P] fp32, S [P] fp64, visits [P] (references taken up, at most 2 F) and terms [P] (terms added)"""
    pts = np.asarray(points, f32).astype(f64).reshape(-1, 3)
    fin = np.isfinite(pts).all(1)
    p = np.where(fin[:, None], pts, 0.0)
    ok, tri = valid_faces(vertices, faces)
    F, P = len(ok), len(p)
    left, right, _ = _refs(nodes)
    mom = np.asarray(mom, f64)
    beta2 = f64(f32(beta)) * f64(f32(beta))
    S, visits, terms = np.zeros(P), np.zeros(P, np.int64), np.zeros(P, np.int64)
    cur = np.full(P, 0 if F > 1 else ~0, np.int64)
    sp, stack = np.zeros(P, np.int64), np.zeros((P, MAX_DEPTH), np.int64)
    live = fin.copy() if F else np.zeros(P, bool)
    with np.errstate(all="ignore"):
        while live.any():
            live &= visits < 2 * F
            idx = np.nonzero(live)[0]
            if not len(idx):
                break
            visits[idx] += 1
            c = cur[idx]
            pop = np.ones(len(idx), bool)
            isn = (c >= 0) & (c < F - 1)
            n, cn = idx[isn], c[isn]
            if len(n):
                x = mom[cn, 0:3] - p[n]
                d2 = dot(x, x)
                far = (d2 > 0.0) & (d2 >= beta2 * mom[cn, 3])
                t = dot(mom[cn, 4:7], x) / (d2 * np.sqrt(d2))
                S[n[far]] += t[far]
                terms[n[far]] += 1
                nn, cnn = n[~far], cn[~far]
                room = sp[nn] < MAX_DEPTH
                stack[nn[room], sp[nn[room]]] = right[cnn[room]]
                sp[nn[room]] += 1
                cur[nn] = left[cnn]
                pop[np.nonzero(isn)[0][~far]] = False
            isl = c < 0
            l, fl = idx[isl], ~c[isl]
            good = fl < F
            good[good] = ok[fl[good]]
            l, fl = l[good], fl[good]
            if len(l):
                S[l] += solid_angle(p[l], tri[fl, 0], tri[fl, 1], tri[fl, 2])
                terms[l] += 1
            q = idx[pop]
            empty = sp[q] == 0
            live[q[empty]] = False
            r = q[~empty]
            sp[r] -= 1
            cur[r] = stack[r, sp[r]]
    return dict(w=_finish(S, fin), S=S, visits=visits, terms=terms)


def host_tree(vertices, faces):
    """(nodes, moments) of test_bvh_cpu.py's host-built Morton tree over the padded boxes"""
    s = bvh_spec()
    lo, hi = s.tri_boxes(vertices, faces)
    nodes = s.build_tree(lo, hi)
    return nodes, moments(nodes, vertices, faces)


# ------------------------------------------------------------------------------------------------- meshes and points
def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], f32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)


def icosphere(level=3, radius=None, centre=None):
    s = bvh_spec()
    return s.spec.icosphere(level, s.RADIUS if radius is None else radius, s.CENTRE if centre is None else centre)


def open_sphere(level=3):
    """the icosphere without the faces whose centroid lies in the cap z > centre + 0.6 radius"""
    s = bvh_spec()
    v, f = icosphere(level)
    zc = v[f].astype(f64).mean(1)[:, 2]
    return v, f[zc <= s.CENTRE[2] + 0.6 * s.RADIUS].copy()


@functools.lru_cache(None)
def scenes():
    """name -> (vertices, faces, closed): the closed and open meshes of the error table"""
    s = bvh_spec()
    iv, ifc = icosphere()
    ov, of = icosphere(2, 0.5 * s.RADIUS)
    cv, cf = md.cube()
    out = {"tetrahedron": tetrahedron() + (True,), "cube": (cv, cf, True), "ico3": (iv, ifc, True),
           "ico4": icosphere(4) + (True,),
           "nested": (np.concatenate([iv, ov]), np.concatenate([ifc, of + len(iv)]).astype(np.int32), True),
           "triangle": (np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], f32), np.array([[0, 1, 2]], np.int32), False),
           "cube pair": (cv, cf[2:4].copy(), False), "open sphere": open_sphere() + (False,)}
    for name in ("soup", "fan"):
        out[name] = s.scenes()[name] + (False,)
    return out


def sample_points(vertices, faces, count, seed=11):
    """count deterministic fp32 points for a mesh: 60 % in its box grown by a quarter of its size, 40 % beside the surface -
    a point of a face moved along that face's normal by +-1e-3 .. 1e-1 of the size"""
    ok, tri = valid_faces(vertices, faces)
    tri = tri[ok]
    rng = np.random.default_rng(seed)
    corners = tri.reshape(-1, 3)
    lo, hi = corners.min(0), corners.max(0)
    size = float((hi - lo).max())
    near = (2 * count) // 5
    box = rng.uniform(lo - 0.25 * size, hi + 0.25 * size, (count - near, 3))
    t = tri[rng.integers(0, len(tri), near)]
    on = (t * rng.dirichlet([1, 1, 1], near)[:, :, None]).sum(1)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    off = size * 10.0 ** rng.uniform(-3, -1, near) * rng.choice([-1.0, 1.0], near)
    return np.concatenate([box, on + n * off[:, None]]).astype(f32)


@functools.lru_cache(None)
def query_points(name):
    """the 1000 points of scene `name`"""
    v, f, _ = scenes()[name]
    return sample_points(v, f, 1000)
