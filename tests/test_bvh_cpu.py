"""numpy fp32 restatement of the BVH tracing contract (include/panonerf_hip.h, "mesh tracing through a device-built BVH"):
padded triangle boxes, the box test with its slab branch and outward rounding, the candidate rule and the closest /
any-hit results; a checker for node buffers; a host-side builder and walker that show the result does not depend on the
tree.  The ray / triangle test, the meshes and the ray helpers are test_objects_cpu.py's.  test_gpu_bvh.py checks the
kernels against this file.

The condition that makes "BVH == brute force" a theorem on a scene is that no (ray, face) pair the ray / triangle test
accepts fails the candidate rule; test_no_accepted_pair_is_lost asserts it, at zero pairs, on the named scenes."""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("_objects_spec_for_bvh",
                                               os.path.join(os.path.dirname(__file__), "test_objects_cpu.py"))
spec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spec)

f32 = np.float32
PAD_REL, PAD_ABS = f32(1e-4), f32(4e-6)  # PN_BVH_PAD_REL, PN_BVH_PAD_ABS
SHRINK, GROW = f32(1.0 - 2.0 ** -21), f32(1.0 + 2.0 ** -21)
KEY_BITS, MAX_DEPTH, NONE = 63, 94, -2 ** 31  # PN_BVH_KEY_BITS, PN_BVH_MAX_DEPTH, PN_BVH_NONE
CENTRE, RADIUS, EYE = np.array([0.5, -0.1, 0.8]), 0.35, (0.02, 0.01, -0.03)  # test_gpu_objects.py's


# -------------------------------------------------------------------------------------------------------------- boxes
def _valid(vertices, faces):
    fc = np.asarray(faces, np.int64)
    return ((fc >= 0) & (fc < len(vertices))).all(1) if len(fc) else np.zeros(0, bool)


def tri_boxes(vertices, faces):
    """(lo [F, 3], hi [F, 3]) fp32: min / max of the three vertices widened by fl(fl(REL ext) + fl(ABS mag)); the empty box
    (+inf, -inf) for a face with an index outside [0, V) or a vertex that is not finite."""
    vt, fc = np.asarray(vertices, f32), np.asarray(faces, np.int64)
    F = fc.shape[0]
    lo, hi = np.full((F, 3), np.inf, f32), np.full((F, 3), -np.inf, f32)
    ok = _valid(vt, fc)
    tri = vt[np.where(ok[:, None], fc, 0)] if F else np.zeros((0, 3, 3), f32)
    ok &= np.isfinite(tri).all((1, 2))
    with np.errstate(all="ignore"):
        l, h = tri.min(1), tri.max(1)
        ext = (h - l).max(1)
        mag = np.abs(tri).max((1, 2))
        pad = (PAD_REL * ext + PAD_ABS * mag).astype(f32)[:, None]
        lo[ok], hi[ok] = (l - pad)[ok], (h + pad)[ok]
    return lo, hi


def box_test(o, d, lo, hi):
    """o, d [R, 3], lo, hi [B, 3] fp32 -> (passed [R, B] bool, tn [R, B] fp32), the header's box test."""
    o, d = np.asarray(o, f32)[:, None, :], np.asarray(d, f32)[:, None, :]
    lo, hi = np.asarray(lo, f32)[None], np.asarray(hi, f32)[None]
    with np.errstate(all="ignore"):
        finite = (np.isfinite(o) & np.isfinite(d)).all(-1)  # [R, 1]
        inv = f32(1) / d
        slab = ~(np.abs(inv) < np.inf)
        a, b = (lo - o) * inv, (hi - o) * inv
        inside = (lo <= o) & (o <= hi)
        near = np.where(slab, -np.inf, np.minimum(a, b)).astype(f32)
        far = np.where(slab, np.inf, np.maximum(a, b)).astype(f32)
        axis_ok = (~slab | inside).all(-1)
        tn, tf = near.max(-1), far.min(-1)
        tn = np.where(tn > 0, tn * SHRINK, tn * GROW).astype(f32)
        tf = np.where(tf > 0, tf * GROW, tf * SHRINK).astype(f32)
        passed = finite & (lo[..., 0] <= hi[..., 0]) & axis_ok & (tn <= tf) & (tf >= 0)
    return passed, tn


# ------------------------------------------------------------------------------------------------ ray / triangle pairs
def mt_pairs(o, d, vertices, faces, t_max=None):
    """(t, u, v, hit) [R, F] fp32: spec.trace's arithmetic for every pair (it returns the winners only); a face with an
    index outside [0, V) is the all-zero triangle, as in the kernel's tris rows."""
    o, d, vt = np.asarray(o, f32)[:, None, :], np.asarray(d, f32)[:, None, :], np.asarray(vertices, f32)
    fc = np.asarray(faces, np.int64)
    ok = _valid(vt, fc)
    tri = np.where(ok[:, None, None], vt[np.where(ok[:, None], fc, 0)], f32(0))
    v0, e1, e2 = tri[None, :, 0], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
    dot = lambda a, b: a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]
    cross = lambda a, b: np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                   a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    eps, one = f32(spec.EDGE_EPS), f32(1)
    with np.errstate(all="ignore"):
        p = cross(d, e2)
        det = dot(e1, p)
        inv = one / det
        s = o - v0
        u = dot(s, p) * inv
        q = cross(s, e1)
        v = dot(d, q) * inv
        t = dot(e2, q) * inv
        hit = (det != 0) & (t > 0) & (t < np.inf) & (u >= -eps) & (v >= -eps) & (u + v <= one + eps)
        if t_max is not None:
            hit &= t < np.asarray(t_max, f32)[:, None]
    assert t.dtype == f32 and u.dtype == f32
    return t, u, v, hit


def candidate_trace(origins, directions, vertices, faces, t_max=None, chunk=1024):
    """The contract's results on every ray: (t [R] (+inf), face [R] (-1), bary [R, 2] fp32, lost, accepted) - the
    lexicographic minimum of (t, f) over the candidates (accepted by the ray / triangle test, the ray passes the face's own
    padded box, tn_f <= t_f).  lost = the pairs the ray / triangle test accepts that are no candidates; accepted = all it
    accepts.  any_hit is face >= 0."""
    o, d = np.asarray(origins, f32), np.asarray(directions, f32)
    R = o.shape[0]
    T, Fi, B = np.full(R, np.inf, f32), np.full(R, -1, np.int32), np.zeros((R, 2), f32)
    lost = accepted = 0
    if not len(faces) or not len(vertices):
        return T, Fi, B, 0, 0
    lo, hi = tri_boxes(vertices, faces)
    for first in range(0, R, chunk):
        sl = slice(first, min(first + chunk, R))
        t, u, v, hit = mt_pairs(o[sl], d[sl], vertices, faces, None if t_max is None else np.asarray(t_max, f32)[sl])
        passed, tn = box_test(o[sl], d[sl], lo, hi)
        cand = hit & passed & (tn <= t)
        lost += int((hit & ~cand).sum())
        accepted += int(hit.sum())
        tt = np.where(cand, t, np.inf).astype(f32)
        j = np.argmin(tt, 1)  # the first minimum: the lowest face index among equal t
        r = np.arange(tt.shape[0])
        ok = cand[r, j]
        T[sl], Fi[sl] = np.where(ok, tt[r, j], np.inf), np.where(ok, j, -1)
        B[sl, 0], B[sl, 1] = np.where(ok, u[r, j], 0), np.where(ok, v[r, j], 0)
    return T, Fi, B, lost, accepted


# ------------------------------------------------------------------------------------------------------------- scenes
def scenes():
    """name -> (vertices fp32, faces int32): a closed mesh, a seeded soup, slivers, two coincident triangles (and the same
    triangle once more with its vertices rotated), a fan that shares edges around a hub."""
    rng = np.random.default_rng(0)
    out = {"ico3": spec.icosphere(3, RADIUS, CENTRE)}
    sv = rng.uniform(-1, 1, (600, 3))
    out["soup"] = (sv.astype(f32), rng.integers(0, 600, (1500, 3)).astype(np.int32))
    dv = np.concatenate([sv[:100], sv[:100] + 1e-6 * rng.normal(size=(100, 3))])
    i = np.arange(100)
    out["sliver"] = (dv.astype(f32), np.stack([i, i + 100, (i + 1) % 100], 1).astype(np.int32))
    tri = CENTRE + 0.3 * np.array([[-1.0, -0.6, 0.1], [1.0, -0.5, -0.2], [0.1, 0.9, 0.15]])
    out["coincident"] = (tri.astype(f32), np.array([[0, 1, 2], [0, 1, 2], [1, 2, 0]], np.int32))
    ang = np.linspace(0, 2 * np.pi, 9)[:-1]
    rim = CENTRE + 0.3 * np.stack([np.cos(ang), np.sin(ang), 0.2 * np.cos(3 * ang)], 1)
    fan_v = np.concatenate([CENTRE[None] + [[0, 0, 0.05]], rim])
    out["fan"] = (fan_v.astype(f32), np.array([[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)], np.int32))
    return out


def scene_rays(vertices, faces, seed=1):
    """(origins, directions) fp32 fired at one mesh: 64 x 128 panoramic rays from EYE, panoramic rays from inside
    (CENTRE), pinhole rays, rays from EYE at every vertex and every edge midpoint, axis-aligned rays with exact zero
    components (through the mesh's box, and through vertices), and origins inside the triangles' boxes and on the
    surface."""
    rng = np.random.default_rng(seed)
    vt = np.asarray(vertices, np.float64)
    tv = vt[np.asarray(faces, np.int64)]  # [F, 3, 3]
    sets = [spec.pano_rays(64, 128, EYE), spec.pano_rays(32, 64, CENTRE),
            spec.pinhole_rays(60, 80, 60.0, spec.look_at(EYE, CENTRE))]
    targets = np.concatenate([vt, ((tv + np.roll(tv, 1, 1)) / 2).reshape(-1, 3)])
    eye = np.broadcast_to(np.asarray(EYE, np.float64), targets.shape).copy()
    sets.append((eye, targets - eye))
    lo, hi = vt.min(0), vt.max(0)
    n = 1500
    ax = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], (n, 1))
    oa = rng.uniform(lo - 0.2, hi + 0.2, (n, 3))
    sets.append((oa, ax))
    k = rng.integers(0, len(targets), 600)  # axis-aligned rays through vertices and edge midpoints
    ax2 = np.eye(3)[rng.integers(0, 3, 600)] * rng.choice([-1.0, 1.0], (600, 1))
    sets.append((targets[k] - 0.75 * ax2, ax2))
    cen = tv.mean(1)
    pick = rng.integers(0, len(cen), 400)
    dirs = rng.normal(size=(400, 3))
    sets.append((cen[pick] + 1e-5 * rng.normal(size=(400, 3)), dirs))  # inside the padded boxes
    sets.append((cen[pick].astype(f32).astype(np.float64), -dirs))  # on the surface, as fp32 sees it
    sets.append((vt[rng.integers(0, len(vt), 200)], rng.normal(size=(200, 3))))  # on a vertex
    o = np.concatenate([s[0] for s in sets]).astype(f32)
    d = np.concatenate([s[1] for s in sets]).astype(f32)
    return o, d


# -------------------------------------------------------------------------------------------------------------- trees
def _refs(nodes):
    n = np.ascontiguousarray(nodes, f32).view(np.int32)
    return n[:, 3], n[:, 7], n[:, 11]


def check_tree(nodes, F, lo=None, hi=None):
    """A node buffer [max(F - 1, 1), 16] is a tree over the faces 0 .. F - 1: every face sits in exactly one leaf, every
    internal node is reached exactly once from the root (row 0) and names its parent, every child box stored in a row is
    the union of the boxes the child's own row stores (and, with lo / hi, a leaf's box is its face's padded box), and no
    leaf lies under more than MAX_DEPTH internal nodes.  -> the largest number of internal nodes above a leaf."""
    nodes = np.ascontiguousarray(nodes, f32)
    assert nodes.shape == (max(F - 1, 1), 16), nodes.shape
    left, right, parent = _refs(nodes)
    box = lambda i, side: (nodes[i, 0:3], nodes[i, 4:7]) if side == 0 else (nodes[i, 8:11], nodes[i, 12:15])
    assert not np.isnan(nodes[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]]).any()
    if F == 1:
        assert left[0] == ~0 and right[0] == NONE and parent[0] == -1
        assert nodes[0, 8] > nodes[0, 12]  # the right side is empty
        if lo is not None:
            assert np.array_equal(nodes[0, 0:3], lo[0]) and np.array_equal(nodes[0, 4:7], hi[0])
        return 1
    seen_face, seen_node = np.zeros(F, np.int64), np.zeros(F - 1, np.int64)
    assert parent[0] == -1
    stack, deepest = [(0, 1)], 0
    seen_node[0] = 1
    while stack:
        i, depth = stack.pop()
        assert depth <= MAX_DEPTH, depth
        for side, ref in ((0, int(left[i])), (1, int(right[i]))):
            blo, bhi = box(i, side)
            if ref < 0:
                f = ~ref
                assert 0 <= f < F, (i, ref)
                seen_face[f] += 1
                deepest = max(deepest, depth)
                if lo is not None:
                    assert np.array_equal(blo, lo[f]) and np.array_equal(bhi, hi[f]), (i, f)
            else:
                assert ref < F - 1 and parent[ref] == i, (i, ref)
                seen_node[ref] += 1
                (l0, h0), (l1, h1) = box(ref, 0), box(ref, 1)
                assert np.array_equal(blo, np.minimum(l0, l1)) and np.array_equal(bhi, np.maximum(h0, h1)), (i, ref)
                stack.append((ref, depth + 1))
    assert (seen_face == 1).all(), np.nonzero(seen_face != 1)[0][:8]
    assert (seen_node == 1).all(), np.nonzero(seen_node != 1)[0][:8]
    return deepest


def morton_keys(lo, hi):
    """63-bit keys of the box centres on a 2^21 grid over the union of the boxes (x the most significant bit of each
    triple); 2^63 - 1 for an empty box."""
    ok = lo[:, 0] <= hi[:, 0]
    keys = np.full(len(lo), 2 ** 63 - 1, np.int64)
    if ok.any():
        slo, shi = lo[ok].min(0).astype(np.float64), hi[ok].max(0).astype(np.float64)
        c = (f32(0.5) * lo[ok] + f32(0.5) * hi[ok]).astype(np.float64)
        w = shi - slo
        with np.errstate(all="ignore"):
            q = np.where(w > 0, (c - slo) / w * 2097152.0, 0.0)
        q = np.clip(np.nan_to_num(q), 0, 2097151).astype(np.int64)
        k = np.zeros(len(q), np.int64)
        for bit in range(21):
            for a in range(3):
                k |= ((q[:, a] >> bit) & 1) << (3 * bit + 2 - a)
        keys[ok] = k
    return keys


def build_tree(lo, hi, keys=None):
    """A radix tree over (key, sorted position) with the node layout of the header, built top-down on the host: the
    topology Karras' kernel finds (rows are numbered in a different order)."""
    F = len(lo)
    nodes = np.zeros((max(F - 1, 1), 16), f32)
    ints = nodes.view(np.int32)
    if F == 1:
        nodes[0, 0:3], nodes[0, 4:7], nodes[0, 8:11], nodes[0, 12:15] = lo[0], hi[0], np.inf, -np.inf
        ints[0, 3], ints[0, 7], ints[0, 11] = ~0, NONE, -1
        return nodes
    keys = morton_keys(lo, hi) if keys is None else np.asarray(keys, np.int64)
    order = np.argsort(keys, kind="stable")
    aug = [(int(keys[order[j]]) << 31) | j for j in range(F)]  # 94-bit strings, all distinct
    count = [0]

    def make(a, b, parent):  # sorted positions a .. b (inclusive) -> (ref, lo, hi)
        if a == b:
            f = int(order[a])
            return ~f, lo[f], hi[f]
        i = count[0]
        count[0] += 1
        top = (aug[a] ^ aug[b]).bit_length() - 1  # the highest bit in which the range differs
        g = a
        while not (aug[g + 1] >> top) & 1:  # the last position whose bit is 0
            g += 1
        ints[i, 11] = parent
        rl, llo, lhi = make(a, g, i)
        rr, rlo, rhi = make(g + 1, b, i)
        nodes[i, 0:3], nodes[i, 4:7], nodes[i, 8:11], nodes[i, 12:15] = llo, lhi, rlo, rhi
        ints[i, 3], ints[i, 7] = rl, rr
        return i, np.minimum(llo, rlo), np.maximum(lhi, rhi)

    make(0, F - 1, -1)
    return nodes


def walk(nodes, F, o, d, vertices, faces, t_max=np.inf, rng=None):
    """The traversal rules of the header for ONE ray, over any node buffer: skip a node only when its box is not passed or
    tn > best; a leaf replaces the best when t < best, or t == best with a face held and f lower.  With rng the order in
    which children are entered is random.  -> (t, face, u, v)."""
    o, d = np.asarray(o, f32)[None], np.asarray(d, f32)[None]
    left, right, _ = _refs(nodes)
    pl, tl = box_test(o, d, nodes[:, 0:3], nodes[:, 4:7])
    pr, tr = box_test(o, d, nodes[:, 8:11], nodes[:, 12:15])
    t, u, v, hit = mt_pairs(o, d, vertices, faces, None if np.isinf(t_max) else np.array([t_max], f32))
    best, face, bu, bv = f32(t_max), -1, f32(0), f32(0)
    stack = [0]
    while stack:
        i = stack.pop()
        todo = []
        for ref, passed, tn in ((int(left[i]), pl[0, i], tl[0, i]), (int(right[i]), pr[0, i], tr[0, i])):
            if not passed or tn > best:
                continue
            if ref >= 0:
                todo.append((tn, ref))
                continue
            f = ~ref
            if hit[0, f] and tn <= t[0, f] and (t[0, f] < best or (t[0, f] == best and face >= 0 and f < face)):
                best, face, bu, bv = t[0, f], f, u[0, f], v[0, f]
        if rng is not None:
            rng.shuffle(todo)
        else:
            todo.sort(reverse=True)  # the near child is popped first
        stack += [ref for _, ref in todo]
    return (best if face >= 0 else f32(np.inf)), face, bu, bv


# -------------------------------------------------------------------------------------------------------------- tests
def test_pairs_are_the_imported_tracer():
    """mt_pairs is spec.trace's arithmetic: its lexicographic winner is spec.trace's result in fp32, bit for bit."""
    v, f = scenes()["ico3"]
    o, d = scene_rays(v, f)
    o, d = o[::7], d[::7]
    t, u, w, hit = mt_pairs(o, d, v, f)
    tt = np.where(hit, t, np.inf).astype(f32)
    j = tt.argmin(1)
    r = np.arange(len(j))
    rt, rface, rbary = spec.trace(o, d, v, f, dtype=f32)
    assert np.array_equal(np.where(hit[r, j], j, -1), rface)
    assert np.array_equal(tt[r, j].view(np.int32), rt.view(np.int32))
    assert np.array_equal(np.where(hit[r, j], u[r, j], 0).astype(f32).view(np.int32), rbary[:, 0].view(np.int32))


@pytest.mark.parametrize("name", ["ico3", "soup", "sliver", "coincident", "fan"])
def test_no_accepted_pair_is_lost(name):
    """With the committed padding no pair the ray / triangle test accepts fails the candidate rule, so on these scenes the
    contract's result IS brute force: checked at zero pairs, and against the imported tracer ray by ray."""
    v, f = scenes()[name]
    o, d = scene_rays(v, f)
    t, face, bary, lost, accepted = candidate_trace(o, d, v, f)
    print(name, "rays", len(o), "faces", len(f), "accepted pairs", accepted, "lost", lost, "hits", int((face >= 0).sum()))
    assert accepted > 500 and (face >= 0).sum() > 200
    assert lost == 0, lost
    rt, rface, rbary = spec.trace(o, d, v, f, dtype=f32)
    assert np.array_equal(face, rface) and np.array_equal(t.view(np.int32), rt.view(np.int32))
    assert np.array_equal(bary.view(np.int32), rbary.view(np.int32))
    tm = np.where(np.arange(len(t)) % 2 == 0, t, t * f32(2)).astype(f32)  # t < t_max is exclusive
    tm[~np.isfinite(tm)] = 1.0
    t2, face2, _, lost2, _ = candidate_trace(o, d, v, f, t_max=tm)
    rt2, rface2, _ = spec.trace(o, d, v, f, t_max=tm, dtype=f32)
    assert lost2 == 0 and np.array_equal(face2, rface2) and np.array_equal(t2.view(np.int32), rt2.view(np.int32))


def test_tighter_padding_loses_pairs():
    """The condition is not empty: without padding, accepted pairs of rays aimed at vertices fall outside their boxes."""
    global PAD_REL, PAD_ABS
    v, f = scenes()["ico3"]
    o, d = scene_rays(v, f)
    keep = PAD_REL, PAD_ABS
    try:
        PAD_REL, PAD_ABS = f32(0), f32(0)
        lost = candidate_trace(o, d, v, f)[3]
    finally:
        PAD_REL, PAD_ABS = keep
    print("lost pairs without padding:", lost)
    assert lost > 0


def test_box_rules():
    lo, hi = np.array([[0, 0, 0], [np.inf] * 3], f32), np.array([[1, 1, 1], [-np.inf] * 3], f32)
    o = np.array([[0.5, 0.5, -1], [0.5, 0.5, -1], [2, 0.5, -1], [1, 0.5, -1], [0.5, 0.5, 0.5], [0.5, 0.5, 2], [np.nan, 0, 0],
                  [0.5, 0.5, -1], [0.5, 0.5, -1]], f32)
    d = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, 1], [1, 1, 1], [0, 0, 1], [0, 0, 1], [0, np.nan, 1],
                  [1e-42, 0, np.inf]], f32)
    passed, tn = box_test(o, d, lo, hi)
    # through; pointing away; a zero component outside the slab; on the slab's face (inclusive); origin inside; behind;
    # NaN origin; NaN direction; infinite direction
    assert passed[:, 0].tolist() == [True, False, False, True, True, False, False, False, False]
    assert not passed[:, 1].any()  # the empty box
    assert tn[0, 0] == f32(1) * SHRINK and tn[4, 0] < 0 and not np.isnan(tn[:6]).any()
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [np.nan, 0, 0]], f32)
    blo, bhi = tri_boxes(v, np.array([[0, 1, 2], [0, 1, 5], [0, 1, 3], [0, -1, 2]], np.int32))
    pad = PAD_REL * f32(2) + PAD_ABS * f32(2)
    assert np.array_equal(blo[0], np.array([0, 0, 0], f32) - pad) and np.array_equal(bhi[0], np.array([1, 2, 0], f32) + pad)
    assert np.isposinf(blo[1:]).all() and np.isneginf(bhi[1:]).all()  # out of range, not finite, negative index


@pytest.mark.parametrize("F", [1, 2, 3, 7, 1280])
def test_host_trees_pass_the_checker(F):
    v, f = spec.icosphere(3, RADIUS, CENTRE)
    f = f[:F]
    lo, hi = tri_boxes(v, f)
    nodes = build_tree(lo, hi)
    depth = check_tree(nodes, F, lo, hi)
    print(F, "depth", depth)
    assert depth <= KEY_BITS + max(F - 1, 1).bit_length()
    if F >= 3:  # the checker notices a wrong box, a face held twice and a lost parent
        for col, row in ((0, 0), (13, F - 2)):
            bad = nodes.copy()
            bad[row, col] += 1.0
            with pytest.raises(AssertionError):
                check_tree(bad, F, lo, hi)
        bad = nodes.copy()
        ints = bad.view(np.int32)
        row = np.nonzero(ints[:, 3] < 0)[0][0]
        ints[row, 3] = ~((~ints[row, 3] + 1) % F)  # another face's leaf
        with pytest.raises(AssertionError):
            check_tree(bad, F)


def test_identical_keys_and_bad_faces_still_give_a_tree():
    """Equal keys are told apart by their sorted position, so 512 triangles with one centroid give a balanced tree of
    depth 9; faces that index outside the vertices sort to the end with empty boxes."""
    rng = np.random.default_rng(2)
    F = 512
    off = rng.normal(size=(F, 3)) * 0.1
    v = np.concatenate([CENTRE + off, CENTRE - off, np.broadcast_to(CENTRE, (F, 3))]).astype(f32)
    f = np.stack([np.arange(F), np.arange(F) + F, np.arange(F) + 2 * F], 1).astype(np.int32)
    lo, hi = tri_boxes(v, f)
    assert check_tree(build_tree(lo, hi, keys=np.zeros(F, np.int64)), F, lo, hi) == 9
    bad = f.copy()
    bad[::5, 2] = len(v) + 3
    lo, hi = tri_boxes(v, bad)
    nodes = build_tree(lo, hi)
    check_tree(nodes, F, lo, hi)
    o, d = scene_rays(v, f[:40])
    t, face, _, _, _ = candidate_trace(o[::9], d[::9], v, bad)
    assert (face >= 0).any() and not np.any(face[face >= 0] % 5 == 0)


@pytest.mark.parametrize("name", ["ico3", "fan", "coincident"])
def test_the_tree_and_the_order_do_not_matter(name):
    """Walking a Morton tree near-child-first, the same tree in random order, and a tree over scrambled keys gives the
    candidate rule's result on every ray, ties and t_max included."""
    v, f = scenes()[name]
    o, d = scene_rays(v, f)
    pick = np.random.default_rng(3).choice(len(o), 160, replace=False)
    o, d = o[pick], d[pick]
    lo, hi = tri_boxes(v, f)
    trees = [build_tree(lo, hi), build_tree(lo, hi, keys=np.random.default_rng(4).integers(0, 2 ** 62, len(f)))]
    for nodes in trees:
        check_tree(nodes, len(f), lo, hi)
    want = candidate_trace(o, d, v, f)
    tm = np.where(np.isfinite(want[0]), want[0], 1).astype(f32)
    want_tm = candidate_trace(o, d, v, f, t_max=tm)
    assert (want[1] >= 0).sum() > 20 and (want_tm[1] >= 0).sum() < (want[1] >= 0).sum()
    rng = np.random.default_rng(5)
    for r in range(len(o)):
        for nodes in trees:
            for order in (None, rng):
                got = walk(nodes, len(f), o[r], d[r], v, f, rng=order)
                assert got[1] == want[1][r] and got[0] == want[0][r] and (got[2], got[3]) == tuple(want[2][r]), (name, r)
        got = walk(trees[0], len(f), o[r], d[r], v, f, t_max=tm[r])
        assert got[1] == want_tm[1][r] and got[0] == want_tm[0][r], (name, r)


def test_accel_argument_checks_that_need_no_device():
    import torch
    from pano_nerf_amd import objects
    z = torch.zeros(4, 3)
    faces = torch.zeros(1, 3, dtype=torch.int32)
    for bad in ("octree", "BVH", 1, True, object()):
        with pytest.raises(ValueError, match="accel must be"):
            objects.trace_mesh(z, z, z, faces, accel=bad)
        with pytest.raises(ValueError, match="accel must be"):
            objects.shadow_ratio(z, z, torch.zeros(3, 4, 8), z, faces, accel=bad)
        with pytest.raises(ValueError, match="accel must be"):
            objects.insert_object(None, None, None, None, accel=bad)
        with pytest.raises(ValueError, match="accel must be"):
            objects.insert_path(None, None, None, None, accel=bad)
    for ok in (None, "bvh"):  # a good accel reaches the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            objects.trace_mesh(z, z, z, faces, accel=ok)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            objects.shadow_ratio(z, z, torch.zeros(3, 4, 8), z, faces, accel=ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objects.MeshBVH.build(z, faces)
    assert hasattr(objects.VirtualObject, "bvh")
