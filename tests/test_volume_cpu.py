"""The numpy restatement of the radiance-volume marcher (tests/_volume_ref.py) held to facts, with no GPU: closed forms in a
constant medium, the SH order against lighting._sh_basis, jump invariance, the pruning bound, the depth rule, the cap on
fragile rays of every scene the GPU tests use, and the file format."""
import functools

import numpy as np
import pytest
import torch

import _cameras_ref as cref
import _volume_ref as ref
import _volume_scenes as scenes


@functools.lru_cache(maxsize=None)
def marched(name, jumps, with_occ, t_min=1e-3, big_step=False):
    data, bounds, deg, _ = scenes.volume(name)
    lo, step = scenes.placement(bounds, data.shape[:3])
    ms = np.float32(2.7 * max(step)) if big_step else scenes.march_step(bounds, data.shape[:3])
    r = scenes.rays()
    occ = ref.occupancy(data) if with_occ else None
    return ref.march(data, lo, step, deg, r["origins"], r["directions"], r["near"], r["far"], ms, t_min, occ, jumps)


def camera_rays(name):
    from pano_nerf_amd import views
    ctor, args = scenes.CAMERAS[name]
    cam = getattr(views, ctor)(*args)
    r = cref.rays(cam, scenes.camera_pose(), scenes.CAMERA_NEAR, scenes.CAMERA_FAR)
    return {k: r[k].astype(np.float32) for k in ("origins", "directions", "near", "far")}


def constant_volume(res, sigma, deg, coeff):
    K = (deg + 1) ** 2
    data = np.zeros(tuple(res) + (1 + 3 * K,), np.float32)
    data[..., 0] = sigma
    data[..., 1:] = np.asarray(coeff, np.float32).reshape(-1)
    return data


def chord(o, d, lo, hi):
    """the length of the ray's intersection with the box (world units), by a slab test in fp64"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    tmin = np.where(d != 0, np.minimum(t0, t1), np.where((o >= lo) & (o <= hi), -np.inf, np.inf)).max(1)
    tmax = np.where(d != 0, np.maximum(t0, t1), np.where((o >= lo) & (o <= hi), np.inf, -np.inf)).min(1)
    return np.maximum(tmax - np.maximum(tmin, 0.0), 0.0) * np.linalg.norm(d, axis=1)


def through_rays(seed, n=64):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(scenes.BOUNDS[0]), np.array(scenes.BOUNDS[1])
    v = rng.standard_normal((n, 3))
    o = 0.5 * (lo + hi) + 1.9 * v / np.linalg.norm(v, axis=1, keepdims=True)
    d = (lo + rng.random((n, 3)) * (hi - lo)) - o
    d *= rng.uniform(0.3, 3.0, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def test_constant_medium_has_the_closed_form():
    c, colour = 3.0, np.array([0.25, 0.5, 1.0])
    res = (5, 6, 7)
    data = constant_volume(res, c, 0, colour / ref.SH_C[0])
    lo, step = scenes.placement(scenes.BOUNDS, res)
    ms = scenes.march_step(scenes.BOUNDS, res)
    o, d = through_rays(1)
    far = (10.0 / np.linalg.norm(d, axis=1)).astype(np.float32)
    got = ref.march(data, lo, step, 0, o, d, 0.0, far, ms, 0.0)
    n = got["evaluated"]
    assert n.min() > 0 and got["marched"].all()
    world = float(ms) * np.ones(len(n))  # dt len, up to an ulp
    np.testing.assert_allclose(got["acc"], 1.0 - np.exp(-c * n * world), rtol=1e-12, atol=1e-14)
    hi64 = lo.astype(np.float64) + step.astype(np.float64) * (np.array(res) - 1)
    L = chord(o.astype(np.float64), d.astype(np.float64), lo.astype(np.float64), hi64)
    assert np.all(np.abs(n * world - L) <= world * (1 + 1e-9))  # the lattice sees the chord to within one step
    assert np.all(got["acc"] <= 1.0 - np.exp(-c * (L + world)) + 1e-12)
    assert np.all(got["acc"] >= 1.0 - np.exp(-c * np.maximum(L - world, 0.0)) - 1e-12)
    np.testing.assert_allclose(got["rgb"], got["acc"][:, None] * data[0, 0, 0, 1:].astype(np.float64) * ref.SH_C[0],
                               rtol=1e-12)
    # the trilinear weights of a constant field sum to 1 within rounding, so the expected distance lies in the chord
    assert np.all((got["depth"] > 0) & (got["depth"] < far))


def test_sh_order_and_constants_are_lightings():
    from pano_nerf_amd import lighting, volume
    rng = np.random.default_rng(3)
    u = rng.standard_normal((50, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    want = lighting._sh_basis(torch.from_numpy(u)).numpy()
    for deg in (0, 1, 2):
        K = (deg + 1) ** 2
        np.testing.assert_allclose(ref.sh_basis(u, deg), want[:, :K], rtol=1e-14, atol=1e-16)
        assert np.array_equal(volume.sh_basis(u, deg), ref.sh_basis(u, deg))
    # a degree-1 volume that encodes a + b . dir renders exactly that function of the view direction
    a, b = np.array([0.9, 0.8, 0.7]), rng.uniform(-0.3, 0.3, (3, 3))  # b[c] is channel c's vector (x, y, z)
    c0, c1 = ref.SH_C[:2]
    coeff = np.stack([a / c0, b[:, 1] / c1, b[:, 2] / c1, b[:, 0] / c1])  # order (0,0) (1,-1)=y (1,0)=z (1,1)=x
    res = (4, 4, 4)
    data = constant_volume(res, 5.0, 1, coeff)
    lo, step = scenes.placement(scenes.BOUNDS, res)
    o, d = through_rays(2)
    got = ref.march(data, lo, step, 1, o, d, 0.0, 10.0, scenes.march_step(scenes.BOUNDS, res), 0.0)
    dirs = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
    stored = data[0, 0, 0, 1:].astype(np.float64).reshape(4, 3)
    a32, b32 = stored[0] * c0, np.stack([stored[3], stored[1], stored[2]], 1) * c1  # what fp32 storage kept of a, b
    assert got["acc"].min() > 0.5
    np.testing.assert_allclose(got["rgb"] / got["acc"][:, None], a32 + dirs @ b32.T, rtol=1e-12)


@pytest.mark.parametrize("name", sorted(scenes.VOLUMES))
def test_jumps_change_no_bit(name):
    plain = marched(name, False, False)
    for with_occ in (False, True):
        jumped = marched(name, True, with_occ)
        for k in ("rgb", "depth", "acc", "attrs", "marched"):
            assert np.array_equal(plain[k], jumped[k], equal_nan=True), (name, with_occ, k)
        assert jumped["evaluated"].sum() <= plain["evaluated"].sum()
    big = marched(name, False, False, 0.0, True), marched(name, True, True, 0.0, True)
    for k in ("rgb", "depth", "acc", "attrs"):
        assert np.array_equal(big[0][k], big[1][k], equal_nan=True), (name, "step > cell", k)


def test_brick_jumps_save_taps_where_bricks_are_empty():
    for name in ("checker", "single"):
        assert marched(name, True, True)["evaluated"].sum() < 0.7 * marched(name, True, False)["evaluated"].sum()


def test_occupancy_of_known_volumes():
    occ = ref.occupancy(scenes.volume("checker")[0])
    i, j, k = np.meshgrid(*[np.arange(2)] * 3, indexing="ij")
    assert np.array_equal(occ, ((i + j + k) % 2 == 0).astype(np.uint8))
    occ = ref.occupancy(scenes.volume("single")[0])
    assert occ.sum() == 1 and occ[1, 1, 1] == 1
    assert ref.occupancy(scenes.volume("partial")[0]).shape == (2, 1, 2)
    nan = scenes.volume("nan")[0].copy()
    nan[..., 0] = np.nan
    assert ref.occupancy(nan).sum() == 0


@pytest.mark.parametrize("name", sorted(scenes.VOLUMES))
def test_fragile_rays_stay_under_the_cap(name):
    for t_min in (0.0, 1e-3, 0.5):
        got = marched(name, False, False, t_min)
        assert got["fragile"].mean() <= 0.01, (name, t_min, int(got["fragile"].sum()))
    assert marched(name, False, False, 0.0, True)["fragile"].mean() <= 0.01


@pytest.mark.parametrize("camera", sorted(scenes.CAMERAS))
def test_fragile_camera_rays_stay_under_the_cap(camera):
    r = camera_rays(camera)
    for name in ("checker", "partial"):
        data, bounds, deg, _ = scenes.volume(name)
        lo, step = scenes.placement(bounds, data.shape[:3])
        got = ref.march(data, lo, step, deg, r["origins"], r["directions"], r["near"], r["far"],
                        scenes.march_step(bounds, data.shape[:3]), 1e-3)
        assert got["fragile"].mean() <= 0.01, (camera, name, int(got["fragile"].sum()))
        assert got["acc"].max() > 0.5  # the frame sees the volume


def test_pruning_removes_at_most_a_hundredth_of_optical_depth():
    rng = np.random.default_rng(8)
    res = (9, 10, 11)
    lo, step = scenes.placement(scenes.BOUNDS, res)
    diag = float(np.linalg.norm(np.array(scenes.BOUNDS[1]) - np.array(scenes.BOUNDS[0])))
    sigma_min = 0.01 / diag
    data = np.zeros(res + (4,), np.float32)
    data[..., 0] = rng.uniform(0.0, 4.0 * sigma_min, res)  # about a quarter of the vertices fall to the threshold
    data[..., 1:] = 1.0
    pruned = data.copy()
    pruned[data[..., 0] <= np.float32(sigma_min)] = 0.0
    assert 0.1 < (pruned[..., 0] == 0).mean() < 0.5
    o, d = through_rays(4, 128)
    ms = scenes.march_step(scenes.BOUNDS, res)
    tau = [-np.log1p(-ref.march(v, lo, step, 0, o, d, 0.0, 10.0, ms, 0.0)["acc"]) for v in (data, pruned)]
    lost = tau[0] - tau[1]
    assert lost.max() > 1e-4  # the rays do cross pruned cells
    assert np.all(lost >= -1e-12) and np.all(lost <= 0.01)


def test_depth_rule():
    data = constant_volume((3, 3, 3), 50.0, 0, np.ones(3))
    lo, step = scenes.placement(scenes.BOUNDS, (3, 3, 3))
    ms = scenes.march_step(scenes.BOUNDS, (3, 3, 3))
    o = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 2.0], [0.0, 0.0, 2.0], [0.0, 0.0, 2.0], [0.0, 0.0, 0.0]], np.float32)
    d = np.array([[0, 0, -1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, -1]], np.float32)
    near = np.array([0.25, 0.25, -1.0, 0.25, 0.0], np.float32)
    far = np.array([4.0, 4.0, 4.0, 4.0, 0.05], np.float32)
    got = ref.march(data, lo, step, 0, o, d, near, far, ms, 0.0)
    assert 1.5 < got["depth"][0] < 1.8 and got["acc"][0] > 0.99  # the surface at z = 0.497 seen from z = 2
    assert got["acc"][1] == 0 and got["depth"][1] == 0.25         # a miss: 0 / 0 -> 0, clamped up to near
    assert got["acc"][2] == 0 and got["depth"][2] == 0.0          # near < 0: the 0 stays
    assert not got["marched"][3] and got["depth"][3] == 0.0       # an invalid row writes 0, not near
    assert got["acc"][4] > 0 and near[4] <= got["depth"][4] <= far[4]


def test_files_round_trip_bit_for_bit(tmp_path):
    from pano_nerf_amd import volume
    data, bounds, deg, attrs = scenes.volume("nan")
    data = data.copy()
    data[0, 0, 0, 1] = -0.0
    volume.write_volume_files(str(tmp_path / "v"), data, bounds, deg, attrs)
    back, b2, d2, a2 = volume.read_volume_files(str(tmp_path / "v"))
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), data.view(np.uint32))
    assert b2 == bounds and d2 == deg and a2 == attrs
    data6, _, deg6, attrs6 = scenes.volume("strides")
    volume.write_volume_files(str(tmp_path / "w"), data6, bounds, deg6, attrs6)
    back, _, _, a2 = volume.read_volume_files(str(tmp_path / "w"))
    assert a2 == (("albedo", 3), ("normal", 3)) and np.array_equal(back, data6)
    with pytest.raises(ValueError):
        volume.write_volume_files(str(tmp_path / "x"), data6, bounds, 2, attrs6)  # C does not match
