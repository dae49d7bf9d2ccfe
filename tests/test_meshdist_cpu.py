"""Holds tests/_meshdist_ref.py, the numpy restatement of the "mesh distance" contract, to facts that need no device:
exact distances, closest points and barycentrics on a dyadic cube from every Voronoi region of a face, the degenerate
faces, the tie-break, the candidate rule (0 violations on every scene test_gpu_meshdist.py uses, with the smallest margin
printed), the properties of systematic sampling, and the argument checks of pano_nerf_amd.meshdist."""
import numpy as np
import pytest

import _meshdist_ref as ref

f32, f64 = np.float32, np.float64

# triangle a = (0, 0, 1), b = (1, 0, 1), c = (0, 1, 1) (face 2 of the cube): (x, y) of the query, the closest point, (u, v)
REGIONS = {
    "vertex a": ((-0.375, -0.5), (0.0, 0.0), (0.0, 0.0)),
    "vertex b": ((1.5, -0.25), (1.0, 0.0), (1.0, 0.0)),
    "vertex c": ((-0.25, 1.5), (0.0, 1.0), (0.0, 1.0)),
    "edge ab": ((0.5, -0.5), (0.5, 0.0), (0.5, 0.0)),
    "edge ac": ((-0.5, 0.25), (0.0, 0.25), (0.0, 0.25)),
    "edge bc": ((1.0, 1.0), (0.5, 0.5), (0.5, 0.5)),
    "interior": ((0.25, 0.25), (0.25, 0.25), (0.25, 0.25)),
}


@pytest.mark.parametrize("region", sorted(REGIONS))
@pytest.mark.parametrize("z", [1.5, 1.0, 0.5])
def test_one_face_from_every_voronoi_region(region, z):
    """above the face's plane (outside the cube), in it and below it (inside): all numbers dyadic, every result exact"""
    v, f = ref.cube()
    (x, y), (qx, qy), (u, w) = REGIONS[region]
    got = ref.closest_point(np.array([[x, y, z]], f32), v, f[2:3])
    want_d2 = (x - qx) ** 2 + (y - qy) ** 2 + (z - 1.0) ** 2
    assert got["face"][0] == 0 and got["d2"][0] == want_d2 and got["distance"][0] == f32(np.sqrt(want_d2))
    assert np.array_equal(got["q"][0], [qx, qy, 1.0]) and np.array_equal(got["uv"][0], [u, w])
    a, b, c = v[f[2]].astype(f64)
    assert np.array_equal((1.0 - u - w) * a + u * b + w * c, got["q"][0])  # bary reproduces closest
    assert got["violations"] == 0


def test_the_whole_cube_outside_inside_and_ties():
    v, f = ref.cube()
    pts = np.array([[0.25, 0.25, 1.5],     # above the top face, over face 2: 0.5
                    [0.75, 0.75, 1.25],    # over face 3: 0.25
                    [-0.375, -0.5, 1.0],   # nearest: the vertex (0, 0, 1), shared by faces 2, 4, 5, 8, 9: the lowest
                    [0.5, -0.75, 2.0],     # nearest: the edge (0, 0, 1) - (1, 0, 1) of faces 2 and 5: 1.25
                    [0.25, 0.25, 0.75],    # inside, under face 2: 0.25
                    [0.5, 0.5, 0.5],       # the centre: 0.5 from all six sides, on the diagonal of each
                    [0.5, 0.25, 0.0],      # on face 0 ... on the surface: 0
                    [1.0, 1.0, 1.0]], f32)  # on the vertex that faces 3, 7 and 11 share
    got = ref.closest_point(pts, v, f)
    assert got["face"].tolist() == [2, 3, 2, 2, 2, 0, 0, 3]
    assert got["d2"].tolist() == [0.25, 0.0625, 0.390625, 1.5625, 0.0625, 0.25, 0.0, 0.0]
    assert got["distance"].tolist() == [0.5, 0.25, 0.625, 1.25, 0.25, 0.5, 0.0, 0.0]
    assert np.array_equal(got["closest"][3], [0.5, 0.0, 1.0]) and np.array_equal(got["closest"][5], [0.5, 0.5, 0.0])
    tri = v[f[got["face"]]].astype(f64)
    u, w = got["uv"][:, 0:1], got["uv"][:, 1:2]
    assert np.array_equal((1.0 - u - w) * tri[:, 0] + u * tri[:, 1] + w * tri[:, 2], got["q"])
    assert got["violations"] == 0
    # coincident faces: the cube twice over; every answer comes from the first copy, and is the single cube's
    twice = ref.closest_point(pts, v, np.concatenate([f, f]))
    assert np.array_equal(twice["face"], got["face"]) and np.array_equal(twice["d2"], got["d2"])
    # max_distance is inclusive, and is squared in fp64 from its fp32 value
    lim = ref.closest_point(pts, v, f, max_distance=0.5)
    assert lim["face"].tolist() == [2, 3, -1, -1, 2, 0, 0, 3] and np.isinf(lim["distance"][[2, 3]]).all()
    assert not lim["closest"][[2, 3]].any() and not lim["bary"][[2, 3]].any()
    assert (ref.closest_point(pts, v, f, max_distance=0.0)["face"] >= 0).tolist() == [False] * 6 + [True] * 2


def test_degenerate_faces():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0.5, 0.5, 0.5]], f32)
    f = np.array([[0, 1, 2]], np.int32)  # three collinear corners: the segments ab, bc, ca
    got = ref.closest_point(np.array([[0.5, 1, 0], [1.5, 1, 0], [3, 0, 1], [-1, 0, 0]], f32), v, f)
    assert got["d2"].tolist() == [1.0, 1.0, 2.0, 1.0]
    assert got["q"].tolist() == [[0.5, 0, 0], [1.5, 0, 0], [2, 0, 0], [0, 0, 0]]
    assert got["uv"].tolist() == [[0.5, 0.0], [0.5, 0.5], [0.0, 1.0], [0.0, 0.0]]
    p = np.array([[0.5, 1, 0], [4, 0, 0]], f32)
    seg = ref.closest_point(p, v, np.array([[0, 1, 1]], np.int32))  # repeated indices: the segment a .. b
    assert seg["d2"].tolist() == [1.0, 9.0] and seg["uv"].tolist() == [[0.5, 0.0], [1.0, 0.0]]
    pt = ref.closest_point(p, v, np.array([[3, 3, 3]], np.int32))  # a point
    assert pt["d2"].tolist() == [0.5, 12.75] and pt["q"].tolist() == [[0.5, 0.5, 0.5]] * 2 and not pt["uv"].any()
    # faces that are never candidates, and the empty mesh
    bad = ref.closest_point(p, v, np.array([[0, 1, 4], [-1, 0, 1]], np.int32))
    assert (bad["face"] == -1).all() and np.isinf(bad["distance"]).all() and bad["violations"] == 0
    vn = v.copy()
    vn[2, 1] = np.nan
    assert ref.closest_point(p, vn, np.array([[0, 1, 2], [0, 1, 3]], np.int32))["face"].tolist() == [1, 1]
    assert (ref.closest_point(p, v, np.zeros((0, 3), np.int32))["face"] == -1).all()
    odd = ref.closest_point(np.array([[np.nan, 0, 0], [0, -np.inf, 0]], f32), v, f)
    assert (odd["face"] == -1).all() and np.isinf(odd["distance"]).all() and not odd["closest"].any()


@pytest.mark.parametrize("name", sorted(ref.meshes()))
def test_no_face_fails_the_candidate_rule(name):
    """Every (finite point, valid face) pair of the GPU file's scenes has lb(p, padded box of f) <= d2(p, f): then every
    valid face is a candidate and the walk's answer is the brute-force answer.  Counted, not trusted."""
    got = ref.answer(name)
    v, f = ref.meshes()[name]
    ok, _ = ref.valid_faces(v, f)
    print(f"{name}: {int(ok.sum())} valid faces of {len(f)}, 998 finite points; violations {got['violations']}; smallest d2 - lb "
          f"of a pair whose point is outside the face's padded box: {got['margin']:.3e}")
    assert got["violations"] == 0
    assert got["margin"] > 0.0
    assert (got["face"][:998] >= 0).all() and (got["face"][998:] == -1).all()
    assert ok[got["face"][:998]].all()


def test_equal_distance_keeps_the_lowest_face_on_the_scenes():
    for name in ("cube", "ico3", "stack"):
        v, f = ref.meshes()[name]
        pts = ref.query_points(name)[:150]  # on vertices: several faces at distance 0
        got = ref.answer(name)
        _, tri = ref.valid_faces(v, f)
        for r in range(0, 150, 7):
            d = ref.point_tri(pts[r].astype(f64)[None, :], tri[:, 0], tri[:, 1], tri[:, 2])[0]
            assert got["d2"][r] == d.min() and got["face"][r] == int(np.argmin(d))


@pytest.mark.parametrize("name,count", [("cube", 1000), ("ico3", 777), ("ico3", 100000), ("sliver fan", 5000), ("bad", 4096),
                                        ("ico3[:3]", 1)])
def test_systematic_sampling(name, count):
    v, f = ref.meshes()[name]
    s = ref.sample_surface(v, f, count)
    w, W = s["weight"], s["W"]
    ok, tri = ref.valid_faces(v, f)
    assert 0 <= int(w.min()) and int(w.max()) == 2 ** 31 and not w[~ok].any() and W == sum(int(x) for x in w) < 2 ** 62
    assert int(s["thresholds"][0]) == 0 and int(s["thresholds"][-1]) < W and (np.diff(s["thresholds"]) >= 0).all()
    got = np.bincount(s["face"], minlength=len(f))
    for k in range(len(f)):  # the floor and the ceiling of the face's share, in exact integers
        lo = count * int(w[k]) // W
        hi = -((-count * int(w[k])) // W)
        assert lo <= got[k] <= hi, (k, lo, got[k], hi)
    # every sample lies in its triangle, and its barycentrics give its point
    u, x = s["uv"][:, 0], s["uv"][:, 1]
    assert (u >= 0).all() and (x >= 0).all() and (u + x <= 1.0).all()
    a, b, c = (tri[s["face"], k] for k in range(3))
    q = (1.0 - u - x)[:, None] * a + u[:, None] * b + x[:, None] * c
    scale = np.abs(tri).max()
    assert np.abs(q - s["q"]).max() <= 4 * 2.0 ** -52 * scale
    assert s["points"].dtype == f32 and s["bary"].dtype == f32 and s["face"].dtype == np.int32


def test_sampling_integers_do_not_overflow():
    """the largest case the header allows: F and count just under 2^31, every weight 2^31"""
    W, count = (2 ** 31 - 1) * 2 ** 31, 2 ** 31 - 1
    i = count - 1
    assert W < 2 ** 62 and i * (W // count) < 2 ** 63 and i * (W % count) < 2 ** 63
    assert i * (W // count) + i * (W % count) // count == i * W // count
    t = ref.thresholds(7 * 2 ** 31 + 12345, 1000)
    assert [int(x) for x in t] == [k * (7 * 2 ** 31 + 12345) // 1000 for k in range(1000)]
    with pytest.raises(ValueError):
        ref.sample_surface(*ref.meshes()["stack"], 10)  # no face has area


def test_argument_checks_that_need_no_device():
    import torch
    from pano_nerf_amd import meshdist
    import pano_nerf_amd as pn
    assert pn.meshdist is meshdist and pn.closest_point is meshdist.closest_point and pn.compare_meshes is meshdist.compare_meshes
    v, f, p = torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(5, 3)
    for bad in ("octree", "BVH", 1, True):
        with pytest.raises(ValueError, match="accel must be"):
            meshdist.closest_point(p, v, f, accel=bad)
        with pytest.raises(ValueError, match="accel must be"):
            meshdist.compare_meshes((v, f), (v, f), accel=bad)
    for bad in (-1.0, float("nan"), "far", torch.zeros(1)):
        with pytest.raises(ValueError, match="max_distance"):
            meshdist.closest_point(p, v, f, max_distance=bad)
        with pytest.raises(ValueError, match="max_distance"):
            meshdist.distance_grid((v, f), ((0, 0, 0), (1, 1, 1)), 4, max_distance=bad)
    for bad in (torch.zeros(5), torch.zeros(5, 2), torch.zeros(5, 3, dtype=torch.float64), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError, match="points must be"):
            meshdist.closest_point(bad, v, f)
    with pytest.raises(ValueError, match="faces must be"):
        meshdist.closest_point(p, v, f.to(torch.int64))
    with pytest.raises(ValueError, match="vertices must be"):
        meshdist.closest_point(p, v[:, :2], f)
    for bad in (0, -3, 2.5, 1 << 31, True):
        with pytest.raises(ValueError, match="count must be"):
            meshdist.sample_surface((v, f), bad)
        with pytest.raises(ValueError, match="samples must be"):
            meshdist.compare_meshes((v, f), (v, f), samples=bad)
    for bad in ((-0.1,), 0.5, ("a",)):
        with pytest.raises(ValueError, match="thresholds must be"):
            meshdist.compare_meshes((v, f), (v, f), thresholds=bad)
    with pytest.raises(ValueError, match="resolution must be"):
        meshdist.distance_grid((v, f), ((0, 0, 0), (1, 1, 1)), 1)
    with pytest.raises(ValueError, match="bounds must be"):
        meshdist.distance_grid((v, f), (0, 1), 4)
    for call in (lambda: meshdist.closest_point(p, v, f), lambda: meshdist.closest_point(p, v, f, accel=None),
                 lambda: meshdist.sample_surface((v, f), 10), lambda: meshdist.compare_meshes((v, f), (v, f)),
                 lambda: meshdist.distance_grid((v, f), ((0, 0, 0), (1, 1, 1)), 4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
