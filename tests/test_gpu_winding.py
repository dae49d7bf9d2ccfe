"""pn_winding.hip on the GPU against tests/_winding_ref.py: the brute-force sum and the Barnes-Hut walk against the numpy
restatement (the walk on the device's own nodes and moments), the moments bit for bit, the walk against brute force on a
deeper tree within the recorded error table, signed distance on a dyadic cube, and remesh of a closed and of an open sphere.

Tolerance of a winding number (derived, not measured): |dw| <= ulp32(|w_ref|) + n 2^-50, n the number of terms (F for brute
force, the visits for the walk).  Both sides run the header's operations in fp64 on the same fp32 inputs in the same order
and round once; every operation but atan2 is IEEE on both sides.  The HIP math API's accuracy table is quoted at 2 ulp for
the fp64 atan2 (the table was not re-read for this test; the bound below has a factor 2 beyond that figure).  A term is at
most 2 pi in magnitude and is divided by 4 pi, so a term of w differs by at most 2 x 2^-53 plus numpy's own last bit, below
2^-51, and the n - 1 additions see operands that differ by that much: n 2^-50 has a factor 2 to spare.  The first term is
the one rounding to fp32, which an fp64 difference may flip.  Seen: 0.50 of the tolerance, the correctly rounded value."""
import numpy as np
import pytest
import torch

import _meshdist_ref as md
import _winding_ref as ref
from _gpu_mesh import N, T, bits_equal, check_w, dev

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64

BRUTE = [f"ico3[:{k}]" for k in (1, 2, 3, ref.TILE - 1, ref.TILE, ref.TILE + 1)] + ["cube", "ico3", "bad", "sliver fan"]


@pytest.mark.parametrize("name", BRUTE)
def test_brute_force_is_the_restatement(name):
    from pano_nerf_amd import winding
    v, f = md.meshes()[name]
    pts = md.query_points(name)  # on vertices, edges and faces, in the box, far away, a NaN row and an inf row
    want = ref.exact(pts, v, f)
    tp, tv, tf = T(pts), T(v), T(f)
    got = winding.winding_number(tp, tv, tf, accel=None)
    assert tuple(got.shape) == (1000,) and got.dtype == torch.float32
    check_w(got, want, len(f), f"{name} brute force")
    assert bits_equal(winding.winding_number(tp, tv, tf, accel=None), got)
    for P in (1, 63, 64, 65):  # the number of points per launch does not show
        assert bits_equal(winding.winding_number(tp[:P], tv, tf, accel=None), got[:P]), P
    assert torch.equal(winding.inside(tp, tv, tf, accel=None), got > 0.5)


@pytest.mark.parametrize("name", ["ico3[:2]", "ico3[:3]", "ico3", "stack", "bad"])
def test_moments_bit_for_bit(name):
    from pano_nerf_amd import objects, winding
    v, f = md.meshes()[name]
    tv, tf = T(v), T(f)
    tree = objects.MeshBVH.build(tv, tf)
    nodes = N(tree.nodes)
    ref.bvh_spec().check_tree(nodes, len(f))
    got = winding._moments(tree, tv, tf, dev())
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(f) - 1, 8)
    assert winding._moments(tree, tv, tf, dev()) is got  # kept on the tree
    want = ref.moments(nodes, v, f)
    same = N(got).view(np.int64) == want.view(np.int64)
    assert same.all(), (name, np.argwhere(~same)[:8])
    again = objects.MeshBVH.build(tv, tf)
    assert bits_equal(again.nodes, tree.nodes) and bits_equal(winding._moments(again, tv, tf, dev()), got)
    if name == "bad":
        assert not np.isnan(want).any()
    if name == "stack":
        assert not want[:, 7].any() and want[:, 3].all()  # faces without area: g is the middle of the box


WALK = [("ico3", b) for b in (1.0, 2.0, 4.0, 8.0, 1e6)] + [("cube", 1.0), ("cube", 4.0), ("ico3[:1]", 4.0), ("ico3[:257]", 2.0),
                                                            ("bad", 2.0), ("bad", 1e6), ("sliver fan", 4.0), ("stack", 2.0)]


@pytest.mark.parametrize("name,beta", WALK)
def test_walk_is_the_restatement_on_the_device_tree(name, beta):
    from pano_nerf_amd import objects, winding
    v, f = md.meshes()[name]
    pts = md.query_points(name)
    tp, tv, tf = T(pts), T(v), T(f)
    tree = objects.MeshBVH.build(tv, tf)
    got = winding.winding_number(tp, tv, tf, accel=tree, beta=beta)
    want = ref.walk(pts, v, f, N(tree.nodes), N(tree._winding_moments), beta)
    assert want["visits"].max() <= 2 * len(f) - 1
    check_w(got, want, want["visits"], f"{name} walk, beta {beta:g} ({want['visits'].mean():.0f} visits per point)")
    assert bits_equal(winding.winding_number(tp, tv, tf, accel="bvh", beta=beta), got)  # a tree built for the call
    assert bits_equal(winding.winding_number(tp, tv, tf, accel=tree, beta=beta), got)
    for P in (1, 63, 65):
        assert bits_equal(winding.winding_number(tp[:P], tv, tf, accel=tree, beta=beta), got[:P]), P
    if beta == 1e6:  # no node is far: the exact sum's terms in another order
        brute = N(winding.winding_number(tp, tv, tf, accel=None)).astype(f64)
        fin = ~np.isnan(brute)
        tol = np.spacing(np.abs(brute[fin]).astype(f32)).astype(f64) + 2 * len(f) * 2.0 ** -50
        assert np.array_equal(np.isnan(N(got)), ~fin) and (np.abs(N(got).astype(f64)[fin] - brute[fin]) <= tol).all()


@pytest.mark.parametrize("beta", [2.0, 4.0, 8.0])
def test_81920_faces_walk_within_the_recorded_error(beta):
    from pano_nerf_amd import objects, winding
    v, f = ref.icosphere(6)
    assert len(f) == 81920
    pts = ref.sample_points(v, f, 4096, seed=13)
    tp, tv, tf = T(pts), T(v), T(f)
    tree = objects.MeshBVH.build(tv, tf)
    walk = winding.winding_number(tp, tv, tf, accel=tree, beta=beta)
    brute = winding.winding_number(tp, tv, tf, accel=None)
    err = float((walk.double() - brute.double()).abs().max())
    closed = float((brute - brute.round()).abs().max())
    print(f"81920 faces, beta {beta:g}: max |w_walk - w_brute| {err:.3e}, recorded E {ref.RECORDED_E[beta]:.3e}; brute force is "
          f"within {closed:.1e} of an integer; {int((brute > 0.5).sum())} of 4096 points inside")
    assert closed < 1e-6  # 81920 terms of fp64 and one rounding
    assert err <= 2.0 * ref.RECORDED_E[beta]
    assert torch.equal(walk > 0.5, brute > 0.5) and 500 < int((brute > 0.5).sum()) < 3500
    assert torch.equal(winding.inside(tp, tv, tf, accel=tree, beta=beta), brute > 0.5)


def test_edge_inputs():
    from pano_nerf_amd import objects, winding
    v, f = md.cube()
    pts = md.query_points("cube")
    tp, tv, tf = T(pts), T(v), T(f)
    fin = torch.isfinite(tp).all(1)
    for vv, ff in ((tv, tf[:0]), (tv[:0], tf)):  # F = 0 and V = 0: zero wherever the point is finite
        for accel in (None, "bvh", objects.MeshBVH.build(vv, ff)):
            w = winding.winding_number(tp, vv, ff, accel=accel)
            assert not bool(w[fin].any()) and bool(torch.isnan(w[~fin]).all()) and int((~fin).sum()) == 2
            d, face, q, b = winding.signed_distance(tp, vv, ff, accel=accel)
            assert bool(torch.isposinf(d).all()) and bool((face == -1).all()) and not bool(q.any()) and not bool(b.any())
    for accel in (None, "bvh"):
        assert tuple(winding.winding_number(tp[:0], tv, tf, accel=accel).shape) == (0,)
        assert [tuple(x.shape) for x in winding.signed_distance(tp[:0], tv, tf, accel=accel)] == [(0,), (0,), (0, 3), (0, 2)]
        w = winding.winding_number(tp, tv, tf, accel=accel)
        assert bool(torch.isnan(w[~fin]).all()) and not bool(winding.inside(tp, tv, tf, accel=accel)[~fin].any())
        d = winding.signed_distance(tp, tv, tf, accel=accel)[0]
        assert bool(torch.isposinf(d[~fin]).all())
    with pytest.raises(ValueError, match="MeshBVH of 12 faces"):
        winding.winding_number(tp, tv, tf[:5], accel=objects.MeshBVH.build(tv, tf))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        winding.winding_number(tp.cpu(), tv, tf)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        winding.inside(tp, tv.cpu(), tf.cpu())
    for bad in (0.5, 0.99, float("nan")):
        with pytest.raises(ValueError, match="beta must be"):
            winding.winding_number(tp, tv, tf, beta=bad)


def cavity():
    """the cube [-2, 3]^3 wound outwards around the unit cube wound inwards: the solid between the two"""
    v, f = md.cube()
    return np.concatenate([v * 5.0 - 2.0, v]).astype(f32), np.concatenate([f, f[:, ::-1] + 8]).astype(np.int32)


# a point in each Voronoi region of the cube's face 2 (a = (0, 0, 1), b = (1, 0, 1), c = (0, 1, 1)), above its plane, and its
# distance to the unit cube: Pythagorean offsets (3, 4, 5) / 8 and (2, 3, 6, 7) / 8, so every value is dyadic and exact
REGION_POINTS = {"vertex a": ((-0.25, -0.375, 1.75), 0.875), "vertex b": ((1.25, -0.375, 1.75), 0.875),
                 "vertex c": ((-0.25, 1.375, 1.75), 0.875), "edge ab": ((0.5, -0.5, 1.375), 0.625),
                 "edge ac": ((-0.5, 0.25, 1.375), 0.625), "edge bc": ((0.5, 0.5, 1.375), 0.375),
                 "interior": ((0.25, 0.25, 1.5), 0.5)}


@pytest.mark.parametrize("accel", [None, "bvh"])
def test_signed_distance_on_the_dyadic_cube(accel):
    """outside the cube the regions' points are outside (+); around the same cube as a cavity of a larger one they are inside
    the solid (-), and the point in the unit cube changes sides the other way"""
    from pano_nerf_amd import winding
    names = sorted(REGION_POINTS)
    pts = np.array([REGION_POINTS[k][0] for k in names] + [(0.25, 0.375, 0.75)], f32)
    want = np.array([REGION_POINTS[k][1] for k in names] + [-0.25])
    v, f = md.cube()
    d, face, q, b = winding.signed_distance(T(pts), T(v), T(f), accel=accel)
    assert N(d).astype(f64).tolist() == want.tolist(), dict(zip(names, N(d)))
    assert N(face)[names.index("edge bc")] == 2 and N(face)[names.index("interior")] == 2
    assert np.array_equal(N(q)[names.index("edge ab")], [0.5, 0.0, 1.0])
    cv, cf = cavity()
    d2, face2, q2, _ = winding.signed_distance(T(pts), T(cv), T(cf), accel=accel)
    assert N(d2).astype(f64).tolist() == (-want).tolist()
    assert np.array_equal(N(face2), N(face) + 12) and bits_equal(q2, q)


@pytest.mark.parametrize("name", ["ico3", "bad"])
def test_signed_distance_is_closest_point_with_the_sign_of_inside(name):
    from pano_nerf_amd import meshdist, objects, winding
    v, f = md.meshes()[name]
    tp, tv, tf = T(md.query_points(name)), T(v), T(f)
    tree = objects.MeshBVH.build(tv, tf)
    fin = np.isfinite(md.answer(name)["distance"])
    md_half = float(np.sort(md.answer(name)["distance"][fin])[fin.sum() // 2])
    for accel in (None, tree, "bvh"):
        for reach in (None, md_half):
            cp = meshdist.closest_point(tp, tv, tf, max_distance=reach, accel=accel)
            ins = winding.inside(tp, tv, tf, accel=accel)
            sd = winding.signed_distance(tp, tv, tf, max_distance=reach, accel=accel)
            assert bits_equal(sd[0], torch.where(ins, -cp[0], cp[0])) and all(bits_equal(a, b) for a, b in zip(sd[1:], cp[1:]))
            assert bits_equal(winding.signed_distance(tp, tv, tf, max_distance=reach, accel=accel)[0], sd[0])
            if name == "ico3":
                assert 50 < int(ins.sum()) < 950 and bool((sd[0][ins] <= 0).all()) and bool((sd[0][~ins] >= 0).all())
            if reach is not None and name == "ico3":
                assert bool(torch.isneginf(sd[0]).any()) and bool(torch.isposinf(sd[0]).any())  # no answer, on either side


def test_grids_are_the_point_queries():
    from pano_nerf_amd import geometry, meshdist, winding
    v, f = ref.icosphere(2)
    mesh = (T(v), T(f))
    lo, hi = v.min(0) - 0.05, v.max(0) + 0.05
    bounds = (tuple(float(x) for x in lo), tuple(float(x) for x in hi))
    res = (9, 12, 10)
    pts = geometry.grid_points(bounds, res)[0]
    for accel in ("bvh", None):
        vol = winding.winding_grid(mesh, bounds, res, accel=accel, beta=3.0)
        assert tuple(vol.shape) == res and vol.dtype == torch.float32 and vol.is_contiguous()
        assert bits_equal(vol.view(-1), winding.winding_number(pts, *mesh, accel=accel, beta=3.0))
        sdf = winding.signed_distance_grid(mesh, bounds, res, accel=accel, beta=3.0)
        assert bits_equal(sdf.abs(), meshdist.distance_grid(mesh, bounds, res))
        assert torch.equal(sdf < 0, vol > 0.5) and 0 < int((sdf < 0).sum()) < sdf.numel()
        lim = winding.signed_distance_grid(mesh, bounds, res, max_distance=0.02, accel=accel, beta=3.0)
        far = sdf.abs() > 0.02
        assert torch.equal(lim[~far], sdf[~far]) and bool(torch.isinf(lim[far]).all()) and torch.equal(lim < 0, sdf < 0)


def check_remesh(out, label):
    from pano_nerf_amd import meshops
    assert out.vertices.dtype == torch.float32 and out.faces.dtype == torch.int32 and out.faces.shape[0] > 0
    edges = meshops.edge_counts(out.faces)
    vlab, flab, count = meshops.mesh_components(out.faces, out.vertices.shape[0])
    stats = meshops.component_stats(out.vertices, out.faces, flab, count)
    print(f"{label}: {out.vertices.shape[0]} vertices, {out.faces.shape[0]} faces, {count} component(s), edges {edges}, "
          f"volume {N(stats['volume']).tolist()}")
    assert edges == {"boundary": 0, "nonmanifold": 0, "inconsistent": 0}
    return count, stats


def test_remesh_of_a_closed_sphere():
    """Every output vertex lies on a tetrahedron edge whose ends have w on either side of 0.5 - on either side of the
    surface, the walk's error being far below 0.5 - so the input surface crosses that edge, and no such edge
    is longer than the cell's diagonal; one ulp of the largest coordinate covers the rounding of the vertex."""
    from pano_nerf_amd import meshdist, winding
    s = ref.bvh_spec()
    v, f = ref.icosphere(3)
    tv, tf = T(v), T(f)
    n = 32
    out = winding.remesh((tv, tf), n)
    count, stats = check_remesh(out, "closed sphere at 32^3")
    assert count == 1
    h = (v.max(0).astype(f64) - v.min(0).astype(f64)) / (n - 5)
    bound = float(np.sqrt((h * h).sum())) + float(np.spacing(f32(np.abs(v).max() + 2 * h.max())))
    d = meshdist.closest_point(out.vertices, tv, tf)[0]
    print(f"  worst distance of an output vertex from the input surface {float(d.max()):.5f}, bound {bound:.5f}")
    assert bool(torch.isfinite(d).all()) and float(d.max()) <= bound
    vol = 4.0 / 3.0 * np.pi * s.RADIUS ** 3
    assert 0.85 * vol < float(stats["volume"][0]) < 1.15 * vol  # outward wound: positive, and the sphere's
    again = winding.remesh((tv, tf), n)
    assert bits_equal(again.vertices, out.vertices) and bits_equal(again.faces, out.faces)
    exact = winding.remesh((tv, tf), n, accel=None)
    assert exact.faces.shape[0] > 0 and check_remesh(exact, "closed sphere, exact sum")[0] == 1


def test_remesh_closes_an_open_sphere():
    from pano_nerf_amd import meshops, winding
    v, f = ref.open_sphere(3)
    tv, tf = T(v), T(f)
    assert meshops.edge_counts(tf)["boundary"] > 0
    out = winding.remesh((tv, tf), 32)
    count, stats = check_remesh(out, "open sphere at 32^3")
    assert count >= 1 and float(stats["volume"].sum()) > 0 and bool((stats["volume"] > 0).all())
