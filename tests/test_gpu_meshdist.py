"""pn_meshdist.hip on the GPU against tests/_meshdist_ref.py: both closest-point kernels against the numpy restatement, the
BVH walk against the brute-force kernel bit for bit, surface sampling, the scores of compare_meshes, distance_grid, and the
end-to-end bound on what simplify_mesh moves.

Tolerance (from the number formats).  Both sides evaluate the header's formulas in fp64 on the same fp32 inputs in the same
order and round once, so the expected distance is 0.5 ulp (0 in bits); every fp32 output is held to ONE fp32 ulp of the
fp64 reference and every integer output exactly.  BVH against brute force has no tolerance: the candidate rule has no
violation on these scenes (test_meshdist_cpu.py), so the two are the same minimum over the same set."""
import numpy as np
import pytest
import torch

import _meshdist_ref as ref

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def dev():
    return torch.device("cuda:0")


def T(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(dev())


def N(x):
    return x.detach().cpu().numpy()


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def same(got, want):
    return all(bits_equal(a, b) for a, b in zip(got, want))


def ulps(got, want):
    """the worst distance of the fp32 `got` from the fp64 `want` in fp32 ulps of `want`; inf where only one is infinite"""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    assert got.shape == want.shape, (got.shape, want.shape)
    both_inf = np.isinf(got) & np.isinf(want) & (got == want)
    with np.errstate(all="ignore"):
        d = np.abs(got - want) / np.spacing(np.abs(want).astype(f32)).astype(f64)
    d = np.where(both_inf, 0.0, d)
    assert not np.isnan(d).any()
    return float(d.max()) if d.size else 0.0


def check_against_ref(got, want, label):
    from conftest import report_worst
    dist, face, closest, bary = (N(x) for x in got)
    assert dist.dtype == f32 and face.dtype == np.int32 and closest.dtype == f32 and bary.dtype == f32
    assert np.array_equal(face, want["face"]), label
    hit = face >= 0
    assert np.isposinf(dist[~hit]).all() and not closest[~hit].any() and not bary[~hit].any()
    wd = np.where(hit, np.sqrt(want["d2"]), np.inf)
    worst = max(ulps(dist, wd), ulps(closest[hit], want["q"][hit]), ulps(bary[hit], want["uv"][hit]))
    print(f"{label}: {int(hit.sum())} answers of {len(face)}, worst distance from the fp64 restatement {worst:.2f} ulp")
    report_worst("closest_point outputs vs the fp64 restatement, fp32 ulp", worst)
    assert worst <= 1.0, (label, worst)


@pytest.mark.parametrize("name", sorted(ref.meshes()))
def test_both_kernels_are_the_restatement_and_each_other(name):
    from pano_nerf_amd import meshdist, objects
    v, f = ref.meshes()[name]
    pts = ref.query_points(name)
    want = ref.answer(name)
    assert want["violations"] == 0
    tp, tv, tf = T(pts), T(v), T(f)
    brute = meshdist.closest_point(tp, tv, tf, accel=None)
    walk = meshdist.closest_point(tp, tv, tf)  # accel="bvh" is the default
    assert tuple(walk[0].shape) == (1000,) and tuple(walk[2].shape) == (1000, 3) and tuple(walk[3].shape) == (1000, 2)
    check_against_ref(brute, want, f"{name} brute force")
    check_against_ref(walk, want, f"{name} BVH")
    assert same(walk, brute)
    # a MeshBVH handed in against one built in the call; two calls give the same bits
    tree = objects.MeshBVH.build(tv, tf)
    assert same(meshdist.closest_point(tp, tv, tf, accel=tree), walk)
    assert same(meshdist.closest_point(tp, tv, tf, accel="bvh"), walk) and same(meshdist.closest_point(tp, tv, tf, accel=None), brute)
    # max_distance at a value that splits the points
    fin = want["distance"][np.isfinite(want["distance"])]
    md = float(np.sort(fin)[len(fin) // 2])
    wl = ref.answer(name, md)
    near = int((wl["face"] >= 0).sum())
    assert 0 < near < 998 and (wl["distance"][wl["face"] >= 0] <= f32(md)).all()
    bl = meshdist.closest_point(tp, tv, tf, max_distance=md, accel=None)
    check_against_ref(bl, wl, f"{name} brute force, max_distance")
    assert same(meshdist.closest_point(tp, tv, tf, max_distance=md, accel=tree), bl)
    # the number of points per launch does not show
    for P in (1, 63, 65, 257):
        assert same(meshdist.closest_point(tp[:P], tv, tf, accel=tree), [x[:P] for x in walk]), P
        assert same(meshdist.closest_point(tp[:P], tv, tf, accel=None), [x[:P] for x in walk]), P


def test_81920_faces_bvh_is_brute_force():
    from pano_nerf_amd import meshdist
    s = ref.bvh_spec()
    v, f = s.spec.icosphere(6, s.RADIUS, s.CENTRE)
    assert len(f) == 81920
    pts = ref.query_points("ico3")  # the same sphere, coarser: points on, inside, around and far from it
    tp, tv, tf = T(pts), T(v), T(f)
    walk = meshdist.closest_point(tp, tv, tf)
    brute = meshdist.closest_point(tp, tv, tf, accel=None)
    assert same(walk, brute)
    d = N(walk[0])
    assert (N(walk[1])[:998] >= 0).all() and np.isinf(d[998:]).all()
    r = np.linalg.norm(pts[:998].astype(f64) - s.CENTRE, axis=1)
    assert np.abs(d[:998] - np.abs(r - s.RADIUS)).max() < 2e-3 * s.RADIUS  # an inscribed level-6 sphere: sagitta ~ 1e-4 R
    md = float(np.median(d[:998]))
    assert same(meshdist.closest_point(tp, tv, tf, max_distance=md), meshdist.closest_point(tp, tv, tf, max_distance=md, accel=None))


def test_edge_inputs():
    from pano_nerf_amd import meshdist, objects
    v, f = ref.meshes()["cube"]
    tp, tv, tf = T(ref.query_points("cube")), T(v), T(f)
    for vv, ff in ((tv, tf[:0]), (tv[:0], tf)):  # F = 0 and V = 0: no answer anywhere
        for accel in (None, "bvh", objects.MeshBVH.build(vv, ff)):
            d, face, q, b = meshdist.closest_point(tp, vv, ff, accel=accel)
            assert bool(torch.isposinf(d).all()) and bool((face == -1).all()) and not bool(q.any()) and not bool(b.any())
    for accel in (None, "bvh"):
        out = meshdist.closest_point(tp[:0], tv, tf, accel=accel)
        assert [tuple(x.shape) for x in out] == [(0,), (0,), (0, 3), (0, 2)]
    with pytest.raises(ValueError, match="MeshBVH of 12 faces"):
        meshdist.closest_point(tp, tv, tf[:5], accel=objects.MeshBVH.build(tv, tf))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshdist.closest_point(tp.cpu(), tv, tf)
    with pytest.raises(ValueError, match="no face with area"):
        meshdist.sample_surface((T(ref.meshes()["stack"][0]), T(ref.meshes()["stack"][1])), 100)
    with pytest.raises(ValueError, match="no face with area"):
        meshdist.sample_surface((tv, tf[:0]), 100)


@pytest.mark.parametrize("name,count", [("cube", 1000), ("ico3", 777), ("ico3", 100000), ("sliver fan", 5000), ("bad", 4097)])
def test_sample_surface_against_the_restatement(name, count):
    from conftest import report_worst
    from pano_nerf_amd import meshdist
    v, f = ref.meshes()[name]
    want = ref.sample_surface(v, f, count)
    got = meshdist.sample_surface((T(v), T(f)), count)
    pts, face, bary = (N(x) for x in got)
    assert pts.dtype == f32 and face.dtype == np.int32 and bary.dtype == f32 and pts.shape == (count, 3) and bary.shape == (count, 2)
    assert np.array_equal(face, want["face"])
    worst = max(ulps(pts, want["q"]), ulps(bary, want["uv"]))
    print(f"{name} x {count}: worst distance from the fp64 restatement {worst:.2f} ulp")
    report_worst("sample_surface outputs vs the fp64 restatement, fp32 ulp", worst)
    assert worst <= 1.0
    assert same(meshdist.sample_surface((T(v), T(f)), count), got)


def test_compare_parallel_quads():
    """two squares with the same footprint h apart: every sample of either is exactly h from the other"""
    from pano_nerf_amd import meshdist
    h = 0.25
    (va, fa), (vb, fb) = ref.quads(h)
    for accel in ("bvh", None):
        s = meshdist.compare_meshes((T(va), T(fa)), (T(vb), T(fb)), samples=3000, thresholds=(0.125, 0.25, 0.5), accel=accel)
        for k in ("accuracy", "completeness", "chamfer", "hausdorff", "hausdorff_ab", "hausdorff_ba", "rms_ab", "rms_ba"):
            assert s[k] == h, (k, s[k])
        assert s["thresholds"] == (0.125, 0.25, 0.5) and s["samples"] == 3000
        assert s["precision"] == (0.0, 1.0, 1.0) and s["recall"] == (0.0, 1.0, 1.0) and s["fscore"] == (0.0, 1.0, 1.0)
        assert abs(s["normal_consistency"] - 1.0) <= 2.0 ** -50


def test_compare_icosphere_with_a_scaled_copy():
    """against the restatement within n 2^-52 max |term|: the bound of an fp64 sum of n terms in any order (each side's sum
    is within n 2^-53 max |term| of the exact mean), not a measurement"""
    from pano_nerf_amd import meshdist
    s = ref.bvh_spec()
    v, f = s.spec.icosphere(2, s.RADIUS, s.CENTRE)
    v2 = (s.CENTRE + 1.0625 * (v.astype(f64) - s.CENTRE)).astype(f32)
    n = 2000
    want = ref.compare_meshes((v, f), (v2, f), n, ())
    taus = (0.01, float(np.median(want["dab"])), 0.03)  # the middle one splits the samples
    want["precision"] = tuple(float((want["dab"] <= t).sum()) / n for t in taus)
    want["recall"] = tuple(float((want["dba"] <= t).sum()) / n for t in taus)
    want["fscore"] = tuple(2 * x * y / (x + y) if x + y > 0 else 0.0 for x, y in zip(want["precision"], want["recall"]))
    got = meshdist.compare_meshes((T(v), T(f)), (T(v2), T(f)), samples=n, thresholds=taus)
    eps = n * 2.0 ** -52
    dmax = max(want["dab"].max(), want["dba"].max())
    assert 0.015 < want["chamfer"] < 0.025 and dmax < 0.03
    for k in ("accuracy", "completeness", "chamfer"):
        assert abs(got[k] - want[k]) <= eps * dmax, (k, got[k], want[k])
    for k in ("rms_ab", "rms_ba"):  # the sums are of d^2; sqrt halves a relative error
        assert abs(got[k] ** 2 - want[k] ** 2) <= eps * dmax * dmax + 4 * 2.0 ** -52 * dmax * dmax, (k, got[k], want[k])
    for k in ("hausdorff_ab", "hausdorff_ba", "hausdorff", "precision", "recall"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert all(abs(a - b) <= 4 * 2.0 ** -52 for a, b in zip(got["fscore"], want["fscore"]))
    assert got["precision"][0] == 0.0 and 0.0 < got["precision"][1] < 1.0 and got["precision"][2] == 1.0
    assert abs(got["normal_consistency"] - want["normal_consistency"]) <= eps + 16 * 2.0 ** -52
    assert want["normal_consistency"] > 0.99


@pytest.mark.parametrize("cells", [2, 4])
def test_simplify_moves_the_surface_by_less_than_a_cell_diagonal(cells):
    """Derived, not measured: a cluster's representative lies in its cell (or is replaced by the mean, which does), so every
    vertex moves by less than the cell's diagonal sqrt(3) cell, and a point of a surviving face moves by the same convex
    combination of its corners' moves.  The image of a surviving face is a face of the simplified mesh, so every sample
    on a surviving face is within sqrt(3) cell of that mesh, plus the fp32 rounding of sample and vertices: one ulp of the
    largest coordinate."""
    from pano_nerf_amd import geometry, meshdist, meshops
    n, R = 48, 0.8
    bounds = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    x = torch.linspace(-1.0, 1.0, n, device=dev())
    gx, gy, gz = torch.meshgrid(x, x + 0.013, x - 0.007, indexing="ij")
    verts, faces = geometry.marching_tetrahedra(R - torch.sqrt(gx * gx + gy * gy + gz * gz), 0.0, bounds)
    cell = cells * 2.0 / (n - 1)
    out, vmap, fmap, flags, info = meshops.simplify_mesh((verts, faces), cell=cell, return_info=True)
    assert 0 < out.faces.shape[0] < faces.shape[0] // cells
    pts, face, _ = meshdist.sample_surface((verts, faces), 20000)
    survives = torch.zeros(faces.shape[0], dtype=torch.bool, device=dev())
    survives[fmap.to(torch.int64)] = True
    keep = survives[face.to(torch.int64)]
    assert int(keep.sum()) >= 100  # most faces of a marching-tetrahedra mesh collapse at 4 grid steps: a few hundred samples remain
    d = meshdist.closest_point(pts[keep], out.vertices, out.faces)[0]
    bound = np.sqrt(3.0) * info["cell"] + float(np.spacing(f32(max(float(verts.abs().max()), float(out.vertices.abs().max())))))
    worst = float(d.max())
    print(f"cell {cells} grid steps = {info['cell']:.5f}: {int(keep.sum())} samples on surviving faces, measured one-sided "
          f"Hausdorff {worst:.5f}, bound sqrt(3) cell + ulp = {bound:.5f}")
    assert bool(torch.isfinite(d).all()) and worst <= bound
    s = meshdist.compare_meshes((verts, faces), out, samples=20000)
    print(f"  all samples: chamfer {s['chamfer']:.5f}, hausdorff {s['hausdorff']:.5f}, normal consistency {s['normal_consistency']:.4f}")
    assert s["chamfer"] < bound


def test_distance_grid_of_the_cube():
    from conftest import report_worst
    from pano_nerf_amd import geometry, meshdist
    v, f = ref.cube()
    bounds = ((-0.5, -0.5, -0.5), (1.5, 1.5, 1.5))  # 17 vertices per axis: a dyadic step of 1 / 8
    vol = meshdist.distance_grid((T(v), T(f)), bounds, 17)
    assert tuple(vol.shape) == (17, 17, 17) and vol.dtype == torch.float32 and vol.is_contiguous()
    pts = N(geometry.grid_points(bounds, 17)[0])
    assert np.array_equal(pts[(3 * 17 + 5) * 17 + 7], f32([-0.125, 0.125, 0.375]))  # density_grid's order
    want = ref.closest_point(pts, v, f)
    worst = ulps(N(vol).reshape(-1), np.sqrt(want["d2"]))
    report_worst("distance_grid vs the fp64 restatement, fp32 ulp", worst)
    assert worst <= 1.0
    assert float(vol[4, 4, 4]) == 0.0 and float(vol[8, 8, 8]) == 0.5 and float(vol[0, 8, 8]) == 0.5 and float(vol[0, 0, 8]) == f32(np.sqrt(0.5))
    lim = meshdist.distance_grid((T(v), T(f)), (bounds[0], (1.5, 1.5, 1.0)), (17, 17, 13), max_distance=0.25)
    assert tuple(lim.shape) == (17, 17, 13)
    assert torch.equal(lim, torch.where(vol[:, :, :13] <= 0.25, vol[:, :, :13], torch.full_like(vol[:, :, :13], float("inf"))))
