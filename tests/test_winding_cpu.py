"""Holds tests/_winding_ref.py, the numpy restatement of the "winding number" contract, to facts that need no device: the
integers of closed meshes, the analytic fractions of open ones, the principal value on the surface, invalid faces, the
properties of the moments, the walk's termination and its beta -> infinity limit, the error table E(beta) of the dipole
approximation (measured against the exact sum, recorded in _winding_ref.RECORDED_E and DESIGN.md 6n), the classification
that follows from it, and the argument checks of pano_nerf_amd.winding."""
import functools

import numpy as np
import pytest

import _winding_ref as ref

f32, f64 = np.float32, np.float64
BETAS = (2.0, 4.0, 8.0)


def plane_sides(pts, v, f):
    """signed distance of every point from the plane of every face of a convex mesh: [P, F], positive outside"""
    tri = v[f].astype(f64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return ((pts[:, None, :] - tri[None, :, 0]) * n[None]).sum(-1)


def known_counts(name):
    """(points, the integer w of each) for a closed scene: the query points that are at least 1e-3 from the surface, by a
    test that does not use solid angles (plane sides of the convex meshes, radii for the spheres)"""
    v, f, closed = ref.scenes()[name]
    assert closed
    pts = ref.query_points(name)
    p = pts.astype(f64)
    s = ref.bvh_spec()
    if name in ("tetrahedron", "cube"):
        d = plane_sides(p, v, f)
        keep = (np.abs(d) >= 1e-3).all(1)  # the nearest surface point lies in one of the planes
        return pts[keep], (d < 0).all(1)[keep].astype(f64)
    r = np.linalg.norm(p - s.CENTRE, axis=1)
    shells = [(v, f)] if name == "ico3" else [(v, f[:1280]), (v, f[1280:])]
    count, keep = np.zeros(len(p)), np.ones(len(p), bool)
    for sv, sf in shells:
        rad = np.linalg.norm(sv[sf].astype(f64) - s.CENTRE, axis=2)
        r_out = rad.max()
        r_in = -plane_sides(s.CENTRE[None], sv, sf).max()  # the inscribed sphere touches the nearest face plane
        assert 0.9 * r_out < r_in < r_out
        keep &= (r < r_in - 1e-3) | (r > r_out + 1e-3)
        count += r < r_in
    return pts[keep], count[keep]


@pytest.mark.parametrize("name", ["tetrahedron", "cube", "ico3", "nested"])
def test_closed_meshes_count_integers(name):
    v, f, _ = ref.scenes()[name]
    pts, want = known_counts(name)
    assert len(pts) > 900 and (want == 1).sum() > 50 and (want == 0).sum() > 50
    if name == "nested":
        assert (want == 2).sum() > 20
    got = ref.exact(pts, v, f)["S"] / ref.FOUR_PI
    worst = np.abs(got - want).max()
    print(f"{name}: {len(pts)} points, worst |w - integer| {worst:.2e}")
    assert worst <= 1e-12
    back = ref.exact(pts, v, f[:, ::-1])["S"] / ref.FOUR_PI  # every face reversed
    assert np.abs(back + want).max() <= 1e-12


def test_open_meshes_give_their_fraction():
    v, f, _ = ref.scenes()["triangle"]
    assert abs(ref.exact(np.zeros((1, 3), f32), v, f)["S"][0] / ref.FOUR_PI - 0.125) <= 1e-12  # one octant of the sphere
    v, f, _ = ref.scenes()["cube pair"]
    assert abs(ref.exact(np.full((1, 3), 0.5, f32), v, f)["S"][0] / ref.FOUR_PI - 1.0 / 6.0) <= 1e-12


def test_points_on_the_surface_take_the_principal_value():
    v, f, _ = ref.scenes()["cube"]
    pts = np.array([[0.5, 0.5, 0.0],    # the centre of a face, on the diagonal its two triangles share
                    [0.25, 0.25, 0.0],  # inside one triangle
                    [0.5, 0.0, 0.0],    # on an edge of the cube: a quarter of the sphere is inside
                    [0.0, 0.0, 0.0],    # on a vertex: an octant
                    [1.5, 0.5, 0.0]], f32)  # in a face's plane, outside the cube
    got = ref.exact(pts, v, f)
    assert np.isfinite(got["w"]).all()
    assert np.abs(got["S"] / ref.FOUR_PI - [0.5, 0.5, 0.25, 0.125, 0.0]).max() <= 1e-12


def test_invalid_faces_and_bad_points():
    v, f, _ = ref.scenes()["ico3"]
    pts = ref.query_points("ico3")[:200].copy()
    want = ref.exact(pts, v, f)
    bv = np.concatenate([v, [[np.nan, 0, 0], [0, np.inf, 0]]]).astype(f32)
    extra = np.array([[0, 1, len(bv)], [-1, 2, 3], [0, 1, len(v)], [len(v) + 1, 5, 6]], np.int32)
    bf = np.concatenate([extra[:2], f[:700], extra[2:], f[700:]])
    got = ref.exact(pts, bv, bf)
    assert np.array_equal(got["S"], want["S"])
    nodes, mom = ref.host_tree(bv, bf)
    assert np.abs(ref.walk(pts, bv, bf, nodes, mom, 1e6)["S"] - want["S"]).max() / ref.FOUR_PI <= len(bf) * 2.0 ** -50
    pts[3, 1], pts[7, 0] = np.nan, np.inf
    got = ref.exact(pts, v, f)["w"]
    assert np.isnan(got[[3, 7]]).all() and np.isfinite(np.delete(got, [3, 7])).all()
    assert not ref.exact(pts, v, f[:0])["w"][[0, 1]].any()  # F = 0: zero


def faces_below(nodes, F):
    """node -> the faces under it, of a node buffer that is a tree"""
    left, right, _ = ref._refs(nodes)
    out = {}

    def below(ref_):
        if ref_ < 0:
            return [~ref_]
        out[ref_] = below(int(left[ref_])) + below(int(right[ref_]))
        return out[ref_]

    below(0)
    return out


@pytest.mark.parametrize("name", ["tetrahedron", "cube", "ico3", "nested", "open sphere", "soup"])
def test_moments(name):
    v, f, closed = ref.scenes()[name]
    nodes, mom = ref.host_tree(v, f)
    g, N, A = ref.leaf_parts(v, f)
    area = A.sum()
    assert abs(mom[0, 7] - area) <= 1e-12 * area
    if closed:
        assert np.abs(mom[0, 4:7]).max() <= 1e-12 * area  # the vector areas of a closed surface cancel
    else:
        assert np.abs(mom[0, 4:7] - N.sum(0)).max() <= 1e-12 * area
    tri = v[f].astype(f64)
    worst = -np.inf
    for node, faces in faces_below(nodes, len(f)).items():
        d2 = ((tri[faces].reshape(-1, 3) - mom[node, 0:3]) ** 2).sum(1).max()
        worst = max(worst, d2 - mom[node, 3])
        assert d2 <= mom[node, 3], (node, d2, mom[node, 3])
    print(f"{name}: {len(f) - 1} nodes, every vertex inside its node's radius (closest margin {-worst:.2e})")


def walk_scenes():
    """test_bvh_cpu.scenes(), 512 triangles under one Morton key, and the same with faces that index outside the vertices"""
    s = ref.bvh_spec()
    out = {k: (v, f, None) for k, (v, f) in s.scenes().items()}
    rng = np.random.default_rng(2)
    F = 512
    off = rng.normal(size=(F, 3)) * 0.1
    v = np.concatenate([s.CENTRE + off, s.CENTRE - off, np.broadcast_to(s.CENTRE, (F, 3))]).astype(f32)
    f = np.stack([np.arange(F), np.arange(F) + F, np.arange(F) + 2 * F], 1).astype(np.int32)
    out["one key"] = (v, f, np.zeros(F, np.int64))
    bad = f.copy()
    bad[::5, 2] = len(v) + 3
    out["bad faces"] = (v, bad, None)
    return out


@pytest.mark.parametrize("name", sorted(walk_scenes()))
def test_walk_ends_and_is_the_exact_sum_for_a_large_beta(name):
    s = ref.bvh_spec()
    v, f, keys = walk_scenes()[name]
    lo, hi = s.tri_boxes(v, f)
    nodes = s.build_tree(lo, hi, keys)
    s.check_tree(nodes, len(f), lo, hi)
    mom = ref.moments(nodes, v, f)
    rng = np.random.default_rng(3)
    pts = rng.uniform(v.min(0) - 0.5, v.max(0) + 0.5, (300, 3)).astype(f32)
    want = ref.exact(pts, v, f)
    F = len(f)
    for beta in (1.0, 4.0, 1e6):
        got = ref.walk(pts, v, f, nodes, mom, beta)
        assert got["visits"].max() <= 2 * F - 1 and got["visits"].min() >= 1
        if beta == 1e6:
            if name != "bad faces":  # no node is far: every reference is taken up (a node of invalid faces only has a
                assert (got["visits"] == 2 * F - 1).all()  # zero row, which is left at once and adds nothing)
            assert np.abs(got["S"] - want["S"]).max() / ref.FOUR_PI <= F * 2.0 ** -50
    # a buffer that is no tree: every row names itself as its left child
    loop = nodes.copy()
    loop.view(np.int32)[:, 3] = np.arange(len(loop))
    got = ref.walk(pts[:10], v, f, loop, mom, 1e6)
    assert (got["visits"] == 2 * F).all() and np.isfinite(got["w"]).all()


@functools.lru_cache(None)
def measured(name, beta):
    """(|w_walk - w_exact| per point in fp64, w_exact, w_walk) of one scene on the host-built tree"""
    v, f, _ = ref.scenes()[name]
    pts = ref.query_points(name)
    nodes, mom = ref.host_tree(v, f)
    exact = ref.exact(pts, v, f)["S"] / ref.FOUR_PI
    walk = ref.walk(pts, v, f, nodes, mom, beta)
    return np.abs(walk["S"] / ref.FOUR_PI - exact), exact, walk["S"] / ref.FOUR_PI, float(walk["visits"].mean())


def test_error_table():
    """E(beta) = max |w_walk - w_exact| over the scenes and their 1000 points each; on the closed scenes w_exact is first
    held to the integers it must be, so the table is measured against facts and the exact fp64 sum, never a kernel.  The
    factor 2 is not for noise (everything here is deterministic): it absorbs last-bit differences of arctan2 between
    libraries and still notices a change of keys or padding that reshapes the tree."""
    E = {}
    print("scene         faces  " + "  ".join(f"E({b:g})      visits" for b in BETAS))
    for name, (v, f, closed) in ref.scenes().items():
        row = []
        for beta in BETAS:
            err, exact, _, visits = measured(name, beta)
            if closed:
                assert np.abs(exact - np.round(exact)).max() <= 1e-9
            E[beta] = max(E.get(beta, 0.0), float(err.max()))
            row.append(f"{err.max():.3e} {visits:7.0f}")
        print(f"{name:13s} {len(f):5d}  " + "  ".join(row))
    print("E(beta):      " + "  ".join(f"{b:g}: {E[b]:.3e} (recorded {ref.RECORDED_E[b]:.3e})" for b in BETAS))
    assert E[8.0] < E[4.0] < E[2.0]
    for beta in BETAS:
        assert E[beta] <= 2.0 * ref.RECORDED_E[beta], (beta, E[beta])


@pytest.mark.parametrize("beta", BETAS)
def test_classification(beta):
    """inside from the walk is inside from the exact sum wherever the exact sum is further than E(beta) from 0.5; on the
    closed scenes that is every point"""
    E = max(float(measured(name, beta)[0].max()) for name in ref.scenes())
    for name, (v, f, closed) in ref.scenes().items():
        _, exact, walk, _ = measured(name, beta)
        clear = np.abs(exact - 0.5) > E
        if closed:
            assert clear.all() and np.abs(np.abs(exact - 0.5) - 0.5)[exact < 1.5].max() < 1e-9
        assert np.array_equal((walk > 0.5)[clear], (exact > 0.5)[clear]), name
        print(f"beta {beta:g}, {name}: {int(clear.sum())} of {len(clear)} points classified, {int((exact > 0.5).sum())} inside")


def test_argument_checks_that_need_no_device():
    import torch
    import pano_nerf_amd as pn
    from pano_nerf_amd import winding
    assert pn.winding is winding and pn.winding_number is winding.winding_number and pn.remesh is winding.remesh
    v, f, p = torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(5, 3)
    grid = ((0, 0, 0), (1, 1, 1))
    for bad in ("octree", "BVH", 1, True):
        for call in (lambda: winding.winding_number(p, v, f, accel=bad), lambda: winding.inside(p, v, f, accel=bad),
                     lambda: winding.signed_distance(p, v, f, accel=bad), lambda: winding.winding_grid((v, f), grid, 4, accel=bad),
                     lambda: winding.remesh((v, f), 8, accel=bad)):
            with pytest.raises(ValueError, match="accel must be"):
                call()
    for bad in (0.5, 0.999, 2e6, float("nan"), float("inf"), -4.0, "4", True, torch.ones(1)):
        for call in (lambda: winding.winding_number(p, v, f, beta=bad), lambda: winding.signed_distance(p, v, f, beta=bad),
                     lambda: winding.signed_distance_grid((v, f), grid, 4, beta=bad), lambda: winding.remesh((v, f), 8, beta=bad)):
            with pytest.raises(ValueError, match="beta must be"):
                call()
    for bad in (-1.0, float("nan"), "far"):
        with pytest.raises(ValueError, match="max_distance"):
            winding.signed_distance(p, v, f, max_distance=bad)
        with pytest.raises(ValueError, match="max_distance"):
            winding.signed_distance_grid((v, f), grid, 4, max_distance=bad)
    for bad in (torch.zeros(5), torch.zeros(5, 2), torch.zeros(5, 3, dtype=torch.float64), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError, match="points must be"):
            winding.winding_number(bad, v, f)
    with pytest.raises(ValueError, match="faces must be"):
        winding.winding_number(p, v, f.to(torch.int64))
    with pytest.raises(ValueError, match="vertices must be"):
        winding.inside(p, v[:, :2], f)
    with pytest.raises(ValueError, match="resolution"):
        winding.winding_grid((v, f), grid, 1)
    for bad in (float("nan"), "half", None):
        with pytest.raises(ValueError, match="level must be"):
            winding.remesh((v, f), 8, level=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        winding.winding_number(p, v, f)


def test_one_number_check_behind_max_distance_beta_and_level():
    """meshdist._number behind _reach, _beta and remesh's level: a bool, a tensor, a NaN and a value out of range raise each
    user's own message, whole; a numpy scalar passes as the fp32 the kernel sees (level: as given)"""
    import torch
    from pano_nerf_amd import meshdist, winding
    v, f = torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32)
    users = {
        "max_distance": (meshdist._reach, "max_distance must be None or a number >= 0", -0.5),
        "beta": (winding._beta, "beta must be a number in [1, 1e6]", 1.5e6),
        "level": (lambda x: winding.remesh((v, f), 8, level=x), "level must be a finite number", float("inf")),
    }
    for name, (call, message, outside) in users.items():
        for bad in (True, torch.ones(1), float("nan"), np.float64("nan"), outside, np.float32(outside)):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(e.value) == f"{message}; got {bad!r}", name
    third = np.float64(1.0) / 3.0
    for good in (np.float32(2.5), np.float64(2.5), np.int64(3), np.float16(1.5), 2, third + 1.0):
        want = float(np.float32(good))
        assert meshdist._reach(good) == want and type(meshdist._reach(good)) is float
        assert winding._beta(good) == want and type(winding._beta(good)) is float
    assert meshdist._reach(None) == float("inf") and meshdist._reach(np.float32("inf")) == float("inf")
    assert meshdist._reach(-1e-50) == 0.0 and winding._beta(1.0 - 1e-9) == 1.0  # judged as fp32
    assert meshdist._number(third, "level", -1.0, 1.0, "", fp32=False) == float(third) != float(np.float32(third))
    assert meshdist._number(1e300, "level", -1.7976931348623157e308, 1.7976931348623157e308, "", fp32=False) == 1e300


def test_the_grid_loop_visits_every_chunk_once(monkeypatch):
    """meshdist._grid_query: first = 0, GRID_CHUNK, ... with the last chunk short, each chunk's answers in its place"""
    import torch
    from pano_nerf_amd import _lib, meshdist
    monkeypatch.setattr(meshdist, "GRID_CHUNK", 7)
    placed, asked = [], []
    grid = (2, 3, 4, 0.0, 0.5, 1.0, 0.25, 0.5, 1.0, 0.0)  # res, lo, step and the radius, as pn_grid_points takes them

    def call(name, *args):
        assert name == "pn_grid_points" and args[:3] + args[5:12] == grid
        placed.append((args[3], args[4]))

    def query(points):
        assert points.shape == (placed[-1][1], 3) and len(asked) == len(placed) - 1
        asked.append(len(points))
        return torch.arange(len(points), dtype=torch.float32) + 100.0 * len(asked)

    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib, "stream", lambda dev: 0)
    vol = meshdist._grid_query(None, torch.device("cpu"), (2, 3, 4), (0.0, 0.5, 1.0), (0.25, 0.5, 1.0), None, query)
    assert placed == [(0, 7), (7, 7), (14, 7), (21, 3)] and asked == [7, 7, 7, 3]
    assert tuple(vol.shape) == (2, 3, 4) and vol.dtype == torch.float32 and vol.is_contiguous()
    want = torch.cat([torch.arange(m, dtype=torch.float32) + 100.0 * (k + 1) for k, m in enumerate(asked)])
    assert torch.equal(vol.view(-1), want)
    placed.clear(), asked.clear()
    grid = (1, 1, 7, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0)
    assert meshdist._grid_query(None, torch.device("cpu"), (1, 1, 7), (0.0,) * 3, (1.0,) * 3, None, query).shape == (1, 1, 7)
    assert placed == [(0, 7)]  # a grid of exactly one chunk: one launch
