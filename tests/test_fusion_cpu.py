"""TSDF fusion without a GPU: the fp64 restatement (tests/_fusion_ref.py) against a closed form, the cap on its fragile
voxels for every scene the GPU tests use, the cull rule and the occupancy conventions on hand-made volumes, and the argument
validation of pano_nerf_amd.fusion (everything raises before the library is touched)."""
import math
import types

import numpy as np
import pytest
import torch

import _fusion_ref as ref
from pano_nerf_amd import _lib, fusion, views


# ------------------------------------------------------------------------------------------------ (a) the closed form
def test_reference_sphere_from_its_centre():
    """A constant-depth R panorama seen from its own eye: sdf = R - rho for every voxel, whatever pixel it lands in, so
    tsdf = min(1, (R - rho) / trunc) exactly where R - rho >= -trunc, and the weight is 0 elsewhere."""
    cam, c2ws, depth, eye, bounds, res = ref.sphere_scene(res=9, R=1.0, half=1.3)
    lo, step = ref.placement(bounds, res)
    trunc = float(np.float32(0.3))
    out = ref.integrate(res, lo, step, cam, c2ws, depth, trunc=trunc)
    rho = np.sqrt(ref.dot(ref.grid(res, lo, step) - ref.f32(eye), ref.grid(res, lo, step) - ref.f32(eye)))
    seen = (1.0 - rho) >= -trunc
    assert seen.any() and (~seen).any() and ((1.0 - rho) / trunc > 1).any()
    assert np.array_equal(out["weight"], seen.astype(np.float64))
    assert np.array_equal(out["tsdf"][seen], np.minimum(1.0, (1.0 - rho) / trunc)[seen])
    assert np.array_equal(out["tsdf"][~seen], np.zeros((~seen).sum()))
    # two views of weight 2 and 0.5: the same mean, the summed weight
    out2 = ref.integrate(res, lo, step, cam, np.concatenate([c2ws, c2ws]), np.concatenate([depth, depth]),
                         view_weights=[2.0, 0.5], trunc=trunc)
    assert np.array_equal(out2["weight"], 2.5 * seen)
    np.testing.assert_allclose(out2["tsdf"], out["tsdf"], rtol=0, atol=1e-15)
    # continuing a volume: the running mean, capped
    out3 = ref.integrate(res, lo, step, cam, c2ws, depth, trunc=trunc, max_weight=1.5, tsdf=out["tsdf"].astype(np.float32),
                         weight=out["weight"].astype(np.float32))
    assert np.array_equal(out3["weight"], 1.5 * seen)
    np.testing.assert_allclose(out3["tsdf"], out["tsdf"], rtol=0, atol=1e-7)


# ------------------------------------------------------------------------------------------------ (b) fragile voxels
def _all_scenes():
    for name, g, n in ref.PARITY:
        cam, c2ws, depth = ref.scene(name, n)
        res, bounds = ref.GRIDS[g]
        yield f"{name}-{g}-{n}", dict(res=res, bounds=bounds, cam=cam, c2ws=c2ws, depth=depth, trunc=ref.TRUNC)
    for name in ("pano", "pinhole"):
        cam, c2ws, depth, conf, vw, dmax, res, bounds = ref.edge_scene(name)
        yield f"edge-{name}", dict(res=res, bounds=bounds, cam=cam, c2ws=c2ws, depth=depth, confidence=conf, view_weights=vw,
                                   depth_max=dmax, trunc=ref.TRUNC)
    cam, c2ws, depth, eye, bounds, res = ref.sphere_scene()
    yield "sphere", dict(res=res, bounds=bounds, cam=cam, c2ws=c2ws, depth=depth, trunc=0.3)


@pytest.mark.parametrize("name,kw", list(_all_scenes()), ids=[n for n, _ in _all_scenes()])
def test_fragile_share_is_capped(name, kw):
    """At most 1 % of the voxels of every scene the GPU tests use hang on a decision an fp64 ulp can flip (a cap, so that
    no GPU test can hide a failure behind the mask), and every scene has voxels in the band, clamped and unseen."""
    kw = dict(kw)
    res, bounds = kw.pop("res"), kw.pop("bounds")
    lo, step = ref.placement(bounds, res)
    out = ref.integrate(res, lo, step, **kw)
    n = out["fragile"].size
    share = out["fragile"].sum() / n
    print(f"{name}: fragile {out['fragile'].sum()} of {n}")
    assert share <= 0.01, (name, share)
    assert out["seen"].any()
    if n > 8:
        assert (~out["seen"]).any() and (np.abs(out["tsdf"][out["seen"]]) < 1).any()


def test_edge_scene_holds_the_edges():
    cam, c2ws, depth, conf, vw, dmax, res, bounds = ref.edge_scene("pano")
    assert np.isnan(depth).any() and (depth == 0).any() and (depth < 0).any() and np.isposinf(depth).any()
    assert (depth[np.isfinite(depth)] > dmax).any() and (conf == 0).any() and np.isnan(conf).any() and vw[-1] == 0
    lo, step = ref.placement(bounds, res)
    X = ref.grid(res, lo, step)
    e = X - c2ws[0, :3, 3]
    assert (np.abs(e).sum(-1) == 0).sum() == 1  # a voxel exactly at the camera centre
    assert ((e[..., 0] == 0) & (e[..., 2] < 0)).any() and ((e[..., 0] == 0) & (e[..., 2] == 0) & (e[..., 1] != 0)).any()
    cam, c2ws, *_ = ref.edge_scene("pinhole")
    back = (X - c2ws[0, :3, 3]) @ c2ws[0, :3, 2]  # along +z of the camera: behind it
    assert (back > 0.1).any() and (np.abs(X - c2ws[0, :3, 3]).sum(-1) == 0).sum() == 1


# --------------------------------------------------------------------------------------------- (c) cull and occupancy
def _volume(res, lo, step, tsdf, weight):
    vol = fusion.TSDFVolume.__new__(fusion.TSDFVolume)
    vol.resolution, vol.lo, vol.step, vol.trunc = res, lo, step, 0.5
    vol.bounds = (lo, tuple(l + s * (n - 1) for l, s, n in zip(lo, step, res)))
    vol.device = torch.device("cuda", 0)
    vol.tsdf, vol.weight = torch.as_tensor(tsdf, dtype=torch.float32), torch.as_tensor(weight, dtype=torch.float32)
    return vol


def test_occupancy_conventions():
    tsdf = np.array([[[0.25, -0.5], [1.0, 0.75]], [[-1.0, 0.125], [0.5, 7.0]]], np.float32)
    weight = np.array([[[1.0, 2.0], [0.0, 0.5]], [[3.0, 0.0], [1.0, 0.0]]], np.float32)
    vol = _volume((2, 2, 2), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), tsdf, weight)
    assert np.array_equal(vol.observed().numpy(), weight > 0)
    solid, empty = vol.occupancy().numpy(), vol.occupancy("empty").numpy()
    assert np.array_equal(solid, np.where(weight > 0, -tsdf, np.float32(1.0)))
    assert np.array_equal(empty, np.where(weight > 0, -tsdf, np.float32(-1.0)))
    assert np.array_equal(vol.occupancy("solid").numpy(), solid)
    with pytest.raises(ValueError, match="unknown"):
        vol.occupancy("hollow")
    with pytest.raises(ValueError, match="unknown"):
        vol.mesh("hollow")


def _cull_numpy(v, f, observed, lo, step):
    """the cull rule as numpy, from its statement"""
    n = observed.shape
    cen = v.astype(np.float64)[f].sum(1) / 3.0
    c = np.floor((cen - np.asarray(lo, np.float64)) / np.asarray(step, np.float64)).astype(np.int64)
    c = np.stack([np.clip(c[:, a], 0, n[a] - 2) for a in range(3)], 1)
    keep = np.ones(len(f), bool)
    for d in np.ndindex(2, 2, 2):
        keep &= observed[c[:, 0] + d[0], c[:, 1] + d[1], c[:, 2] + d[2]]
    f = f[keep]
    used = np.zeros(len(v), bool)
    used[f.reshape(-1)] = True
    return v[used], (np.cumsum(used) - 1)[f].astype(np.int32)


def test_cull_rule_on_hand_made_volumes():
    lo, step = (-1.0, 0.5, 2.0), (0.5, 0.25, 1.0)
    observed = np.ones((4, 3, 3), bool)
    observed[3, 2, 1] = False  # the cells (2, 1, 0) and (2, 1, 1) lose a corner
    p = lambda i, j, k: [lo[0] + i * step[0], lo[1] + j * step[1], lo[2] + k * step[2]]
    v = np.array([p(0.1, 0.1, 0.1), p(0.9, 0.2, 0.3), p(0.2, 0.8, 0.5),      # a face in cell (0, 0, 0): kept
                  p(2.2, 1.3, 0.4), p(2.7, 1.6, 0.2), p(2.4, 1.9, 0.9),      # a face in cell (2, 1, 0): dropped
                  p(2.5, 1.5, 1.5),                                          # with vertices 3 and 4 in cell (2, 1, 0)...
                  p(-0.7, 0.3, 0.2),                                         # a vertex outside the grid: clamps to cell 0
                  p(9.0, 9.0, 9.0)], np.float32)                             # a vertex no face uses
    f = np.array([[0, 1, 2], [3, 4, 5], [3, 4, 6], [7, 0, 1], [2, 1, 0], [1, 2, 4]], np.int32)
    want_v, want_f = _cull_numpy(v, f, observed, lo, step)
    got_v, got_f = fusion.cull_faces(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(observed), lo, step)
    assert got_f.dtype == torch.int32
    assert np.array_equal(got_v.numpy(), want_v) and np.array_equal(got_f.numpy(), want_f)
    assert want_f.tolist() == [[0, 1, 2], [4, 0, 1], [2, 1, 0], [1, 2, 3]]  # order kept; vertices 3 5 6 8 gone, 4 -> 3, 7 -> 4
    assert np.array_equal(want_v, v[[0, 1, 2, 4, 7]])
    # everything observed: nothing changes but the unused vertex; nothing observed: nothing is left
    all_v, all_f = fusion.cull_faces(torch.from_numpy(v), torch.from_numpy(f), torch.ones(4, 3, 3, dtype=torch.bool), lo, step)
    assert np.array_equal(all_f.numpy(), f) and np.array_equal(all_v.numpy(), v[:8])
    no_v, no_f = fusion.cull_faces(torch.from_numpy(v), torch.from_numpy(f), torch.zeros(4, 3, 3, dtype=torch.bool), lo, step)
    assert tuple(no_v.shape) == (0, 3) and tuple(no_f.shape) == (0, 3)


# ------------------------------------------------------------------------------------------------------ (d) arguments
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "call", boom)


BOUNDS = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def test_volume_arguments(no_library):
    for res in (1, (4, 4), (4, 1, 4), 2048):
        with pytest.raises(ValueError, match="resolution"):
            fusion.TSDFVolume(BOUNDS, res, device="cuda")
    for bounds in (((0, 0, 0), (1, 1)), "box", ((0, 0, 0), (1, 0, 1)), ((0, 0, 0), (1, math.nan, 1))):
        with pytest.raises(ValueError, match="bounds"):
            fusion.TSDFVolume(bounds, 4, device="cuda")
    for trunc in (0.0, -1.0, math.inf, math.nan, 1e-60):
        with pytest.raises(ValueError, match="trunc"):
            fusion.TSDFVolume(BOUNDS, 4, trunc=trunc, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fusion.TSDFVolume(BOUNDS, 4, device="cpu")


def test_integrate_arguments(no_library):
    vol = _volume((4, 4, 4), (-1.0, -1.0, -1.0), (0.5, 0.5, 0.5), np.zeros((4, 4, 4)), np.zeros((4, 4, 4)))
    cam, pose = views.pano_camera(8, 16), np.eye(4)
    d = torch.ones(2, 8, 16)
    bad = [
        (dict(depth=np.ones((8, 16))), "depth must be"),
        (dict(depth=torch.ones(16)), "depth must be"),
        (dict(depth=torch.ones(2, 3, 8, 16)), "depth must be"),
        (dict(depth=torch.ones(2, 8, 15)), "camera is 8 x 16"),
        (dict(depth=torch.ones(0, 8, 16)), "empty"),
        (dict(camera=views.stereo_pano_camera(8, 16, 0.06, "left")), "stereo"),
        (dict(camera="pano"), "camera must come from"),
        (dict(c2w=np.eye(4)), "holds 1 poses but depth 2"),
        (dict(c2w=np.ones((2, 2, 2))), "c2w"),
        (dict(confidence=torch.ones(2, 8, 15)), "confidence"),
        (dict(confidence=np.ones((2, 8, 16))), "confidence"),
        (dict(weights=[1.0]), "weights"),
        (dict(depth_max=0.0), "depth_max"),
        (dict(depth_max=math.nan), "depth_max"),
        (dict(max_weight=-1.0), "max_weight"),
    ]
    for change, match in bad:
        kw = dict(depth=d, camera=cam, c2w=np.stack([pose, pose]))
        kw.update(change)
        with pytest.raises(ValueError, match=match):
            vol.integrate(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # every argument is fine, but the depth is a CPU tensor
        vol.integrate(d, cam, np.stack([pose, pose]), confidence=torch.ones(2, 1, 8, 16), weights=[1.0, 2.0], depth_max=math.inf)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.integrate(torch.ones(8, 16), cam, pose)


def test_fuse_arguments(no_library):
    model = types.SimpleNamespace(_NC=5)  # never reached: every call below fails on its arguments first
    cam, poses = views.pano_camera(8, 16), np.stack([np.eye(4)] * 3)
    with pytest.raises(ValueError, match="stereo"):
        fusion.fuse_views(model, views.stereo_pano_camera(8, 16, 0.06, "right"), poses, BOUNDS, 4)
    for g in (0, -1, 1.5):
        with pytest.raises(ValueError, match="views_per_call"):
            fusion.fuse_views(model, cam, poses, BOUNDS, 4, views_per_call=g)
    with pytest.raises(ValueError, match="poses"):
        fusion.fuse_views(model, cam, np.ones((3, 2)), BOUNDS, 4)
    with pytest.raises(ValueError, match="depth_max"):
        fusion.fuse_views(model, cam, poses, BOUNDS, 4, depth_max=0.0)
    with pytest.raises(ValueError, match="confidence"):
        fusion.fuse_views(model, cam, poses, BOUNDS, 4, confidence=torch.ones(2, 8, 16))
    with pytest.raises(ValueError, match="resolution"):
        fusion.fuse_views(model, cam, poses, BOUNDS, 1)
    with pytest.raises(ValueError, match="trunc"):
        fusion.fuse_views(model, cam, poses, BOUNDS, 4, trunc=-0.1)
    with pytest.raises(ValueError, match="bounds"):
        fusion.fuse_views(model, cam, poses, ((0, 0), (1, 1)), 4)
    with pytest.raises(ValueError, match="colors"):
        fusion.fused_mesh(model, cam, poses, BOUNDS, 4, colors="red")
    with pytest.raises(ValueError, match="albedo"):
        fusion.fused_mesh(types.SimpleNamespace(_NC=1), cam, poses, BOUNDS, 4, colors="albedo")
    with pytest.raises(ValueError, match="unknown"):
        fusion.fused_mesh(model, cam, poses, BOUNDS, 4, unknown="void")
    with pytest.raises(ValueError, match="fused_mesh takes"):
        fusion.fused_mesh(model, cam, poses)
    vol = _volume((4, 4, 4), (-1.0, -1.0, -1.0), (0.5, 0.5, 0.5), np.zeros((4, 4, 4)), np.zeros((4, 4, 4)))
    with pytest.raises(ValueError, match="belong to fuse_views"):
        fusion.fused_mesh(model, vol, far=5.0)


def test_exported_from_the_package():
    import pano_nerf_amd as pn
    assert pn.fusion is fusion and pn.TSDFVolume is fusion.TSDFVolume
    assert pn.fuse_views is fusion.fuse_views and pn.fused_mesh is fusion.fused_mesh
    assert "pn_tsdf_integrate" in _lib.SIGNATURES
