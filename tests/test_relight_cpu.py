"""The relighting contract on the CPU: the fp64 restatement of pn_relight (tests/_relight_ref.py) against analytic cases in
its analytic room, the conditions the GPU comparison relies on (almost no row hangs on a decision an fp64 ulp can flip;
every scene exercises dark, lit and partly lit rows), and the host-side validation of pano_nerf_amd.relight.  No GPU."""
import math

import numpy as np
import pytest
import torch

import _cameras_ref as cref
import _relight_ref as ref
from pano_nerf_amd import views


@pytest.fixture(scope="module")
def lights():
    return ref.light_rows()


@pytest.fixture(scope="module")
def results(lights):
    """every scene's reference result, computed once: (view, map, pcf) -> dict"""
    out = {}
    for v in ref.VIEWS:
        rows = ref.view_rows(v)
        for m in ref.MAPS:
            maps = ref.shadow_maps(lights, *m)
            for k in ref.PCFS:
                out[(v, m, k)] = ref.relight(rows, lights, maps, m[0], k)
    return out


def test_scenes_cover_the_issue():
    assert len(ref.SCENES) == 4 * 3 * 3
    assert [len(ref.view_rows(v)["depth"]) for v in ref.VIEWS] == [16 * 32, 17 * 33, 6 * 8 * 8, 16 * 16]
    rows = ref.view_rows("pano")
    assert rows["depth"].dtype == np.float32 and rows["normals"].dtype == np.float32
    assert np.isfinite(rows["depth"]).all() and (rows["depth"] > 0).all() and (rows["sid"] == ref.SPHERE_ID).sum() > 20
    lt = ref.light_rows()
    assert lt.shape == (3, 16) and lt.dtype == np.float32 and not lt[0, 6:9].any() and lt[1, 6:9].any()
    # the third light's clamp is active: some wall point of the panorama view is nearer than its r_min
    X = rows["origins"].astype(np.float64) + rows["depth"][:, None].astype(np.float64) * rows["directions"]
    assert (np.linalg.norm(X - lt[2, :3], axis=1) < lt[2, 11]).sum() >= 3


def test_almost_no_row_is_fragile(results):
    """the condition of the GPU comparison: on every scene at least 99 % of the rows are decided with room to spare"""
    for key, r in results.items():
        share = 1.0 - r["fragile"].mean()
        assert share >= 0.99, (key, share)


def test_every_scene_has_dark_lit_and_partly_lit_rows(results):
    for key, r in results.items():
        V = r["visibility"].astype(np.float32)  # as the kernel stores it
        assert (V == 0).any() and (V == 1).any() and ((V > 0) & (V < 1)).any(), key
        assert np.all((V >= 0) & (V <= 1)), key
        assert np.isfinite(r["out"]).all() and np.isfinite(r["direct"]).all() and (r["direct"] >= 0).all(), key


def test_unoccluded_plane_is_lambert_over_r_squared():
    """a plane under one omni light, nothing in between (an empty map: every texel NaN or far): direct = albedo / pi I cos / r^2"""
    rng = np.random.default_rng(5)
    R = 200
    pts = np.stack([rng.uniform(-1, 1, R), np.zeros(R), rng.uniform(-1, 1, R)], 1)
    o = (pts + np.array([0.3, 2.0, -0.1])).astype(np.float32)
    d = np.broadcast_to(np.array([-0.3, -2.0, 0.1], np.float32), (R, 3)).copy()
    rows = dict(origins=o, directions=d, depth=np.ones(R, np.float32), normals=np.tile(np.float32([0, 2, 0]), (R, 1)),
                albedo=rng.uniform(0.1, 0.9, (R, 3)).astype(np.float32), rgb=rng.uniform(0, 1, (R, 3)).astype(np.float32))
    light = np.zeros((1, 16), np.float32)
    light[0, :3], light[0, 3:6] = (0.2, 0.7, -0.4), (3.0, 1.0, 0.5)
    for maps in (np.full((1, 8, 16), np.nan, np.float32), np.full((1, 8, 16), 50.0, np.float32)):
        r = ref.relight(rows, light, maps, ref.MAP_PANO, 3, ambient=0.5)
        X = o.astype(np.float64) + d.astype(np.float64)
        w = light[0, :3].astype(np.float64) - X
        r2 = (w * w).sum(1)
        cos = w[:, 1] / np.sqrt(r2)
        want = rows["albedo"].astype(np.float64) / math.pi * light[0, 3:6].astype(np.float64) * (cos / r2)[:, None]
        assert np.all(np.abs(r["visibility"] - 1.0) <= 4e-16)  # the four fp64 weights sum to 1 within two roundings
        np.testing.assert_allclose(r["direct"], want, rtol=1e-12, atol=0)
        np.testing.assert_allclose(r["out"], 0.5 * rows["rgb"].astype(np.float64) + want, rtol=1e-12, atol=0)


def test_hard_shadow_is_the_analytic_occlusion_of_the_sphere(lights):
    """pcf = 1 against a fine map (256 x 512, delta = pi / 256) of the omni light, default biases: away from the shadow's
    edge the visibility is the analytic occlusion of the segment light -> point by the sphere.

    "Away from the edge" is decided in the map: the 4 x 4 texels around the lookup (two texels to every side) are all
    sphere or none of them is.  Where none is, they must also all be the row's own surface (a crease of the room is a depth
    edge of its own).  Rows with tan(incidence) <= 3 are checked: there the slope term covers the change of depth over the
    window - a plane at distance z and incidence theta changes by z tan(theta) eps + z (1 + 2 tan^2) eps^2 / 2 over an angle
    eps <= sqrt(2) delta, against the allowance 0.02 z + 0.01 + 2 z delta tan: the first-order terms leave (2 - sqrt 2) delta
    tan z, the second-order term is at most 19 delta^2 z = 0.003 z < 0.02 z; the sphere curves away from its tangent
    plane, which only adds distance.  A row in shadow has rho > 1.02 T + 0.01 + slope with T the tangent length from the
    light to the sphere (no texel on the sphere is farther), which the test asserts of the rows it then requires dark."""
    Hm, Wm = 256, 512
    p = lights[0, :3].astype(np.float64)
    maps, ids = ref.shadow_maps(lights[:1], ref.MAP_PANO, Hm, Wm, with_ids=True)
    T = math.sqrt(((ref.SPHERE_C - p) ** 2).sum() - ref.SPHERE_R ** 2)
    delta = math.pi / Hm
    n_dark = n_lit = 0
    for v in ref.VIEWS:
        rows = ref.view_rows(v)
        r = ref.relight(rows, lights[:1], maps, ref.MAP_PANO, 1)
        V, NoL = r["visibility"][:, 0], r["NoL"][:, 0]
        nh = rows["normals"].astype(np.float64)
        nh = nh / np.maximum(np.linalg.norm(nh, axis=1, keepdims=True), 1e-30)
        X = rows["origins"].astype(np.float64) + rows["depth"][:, None].astype(np.float64) * rows["directions"]
        vec = X + ref.f32(0.02) * nh - p
        rho = np.linalg.norm(vec, axis=1)
        pos = cref.dir_to_pix(views.PanoCamera(Hm, Wm), vec)
        x0, y0 = np.floor(pos["px"] - 0.5).astype(int), np.floor(pos["py"] - 0.5).astype(int)
        with np.errstate(divide="ignore", invalid="ignore"):
            tan = np.sqrt(np.maximum(0, 1 - NoL ** 2)) / NoL
        blocked = ref.occluded(X, p)
        for i in np.nonzero(r["valid"] & (NoL > 0) & (tan <= 3.0))[0]:
            ys = np.clip(np.arange(y0[i] - 1, y0[i] + 3), 0, Hm - 1)
            xs = np.arange(x0[i] - 1, x0[i] + 3) % Wm
            near = ids[0][np.ix_(ys, xs)]
            on_sphere = near == ref.SPHERE_ID
            if on_sphere.all() and rows["sid"][i] != ref.SPHERE_ID:
                assert blocked[i], (v, i)
                assert rho[i] > 1.02 * T + 0.011 + 2.0 * rho[i] * delta * tan[i], (v, i)
                assert V[i] == 0.0, (v, i, V[i])
                n_dark += 1
            elif (near == rows["sid"][i]).all():
                assert not blocked[i], (v, i)
                assert abs(V[i] - 1.0) <= 4e-16, (v, i, V[i], tan[i])
                n_lit += 1
    assert n_dark >= 20 and n_lit >= 500, (n_dark, n_lit)


def test_edge_rows_of_the_restatement():
    """rows with no depth or no normal keep ambient rgb; texels that are no surface light; L = 0 is the ambient image"""
    lights = ref.light_rows()
    rows = {k: v[:40].copy() for k, v in ref.view_rows("pano").items()}
    rows["depth"][:4] = (np.nan, 0.0, -1.0, np.inf)
    rows["normals"][4] = 0.0
    rows["normals"][5, 1] = np.nan
    maps = ref.shadow_maps(lights, ref.MAP_PANO, 8, 16)
    r = ref.relight(rows, lights, maps, ref.MAP_PANO, 3, ambient=0.25)
    assert not r["visibility"][:6].any() and not r["direct"][:6].any()
    assert np.array_equal(r["out"][:6], 0.25 * rows["rgb"][:6].astype(np.float64))
    empty = maps.copy()
    empty[:, ::2] = np.nan
    empty[:, 1::2, ::2] = 0.0
    empty[:, 1::2, 1::2] = -1.0
    r2 = ref.relight(rows, lights[:1], empty[:1], ref.MAP_PANO, 3)
    facing = r2["NoL"][:, 0] > 0
    assert facing.any() and np.all(np.abs(r2["visibility"][facing, 0] - 1.0) <= 4e-16)
    r0 = ref.relight(rows, lights[:0], None, ref.MAP_PANO, 1)
    assert r0["visibility"].shape == (40, 0) and np.array_equal(r0["out"], rows["rgb"].astype(np.float64))


# ------------------------------------------------------------------------------------------------ host-side validation
def test_module_imports_without_a_gpu():
    import pano_nerf_amd as pn
    from pano_nerf_amd import relight as rl
    assert pn.relight is rl
    for name in ("PointLight", "pack_lights", "light_rows", "shadow_maps", "relight", "light_visibility", "relight_view",
                 "relight_path"):
        assert callable(getattr(rl, name)), name
    assert rl.LIGHT_FLOATS == 16 and rl.MAX_PCF == 7


def test_point_light_validation_and_rows():
    from pano_nerf_amd import relight as rl
    a = rl.PointLight((1, 2, 3), 2.0)
    row = a.row()
    assert row.dtype == np.float32 and row.shape == (16,)
    assert row[:6].tolist() == [1, 2, 3, 2, 2, 2] and not row[6:11].any() and row[11] == np.float32(0.05) and not row[12:].any()
    s = rl.PointLight((0, 0, 0), (1, 2, 3), axis=(0, -2, 0), inner_deg=10, outer_deg=30, r_min=0).row()
    assert s[6:9].tolist() == [0, -1, 0] and s[9] == np.float32(math.cos(math.radians(10))) and s[10] == np.float32(math.cos(math.radians(30)))
    assert s[11] == 0 and s[3:6].tolist() == [1, 2, 3]
    assert rl.PointLight((0, 0, 0), 1, axis=(1, 0, 0), inner_deg=0, outer_deg=180).row()[10] == -1
    bad = [dict(position=(0, 0)), dict(position=(0, np.nan, 0)), dict(intensity=-1.0), dict(intensity=(1, 2)),
           dict(intensity=np.inf), dict(r_min=-0.1), dict(r_min=np.nan), dict(inner_deg=10), dict(axis=(0, 0, 0), inner_deg=1, outer_deg=2),
           dict(axis=(1, 0, 0)), dict(axis=(1, 0, 0), inner_deg=30, outer_deg=30), dict(axis=(1, 0, 0), inner_deg=40, outer_deg=30),
           dict(axis=(1, 0, 0), inner_deg=10, outer_deg=181), dict(axis=(1, 0, 0), inner_deg=-1, outer_deg=30),
           dict(axis=(1, np.inf, 0), inner_deg=10, outer_deg=30), dict(axis=(1, 0, 0), inner_deg=np.nan, outer_deg=30)]
    for kw in bad:
        args = dict(position=(0, 0, 0), intensity=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            rl.PointLight(**args)
    with pytest.raises(ValueError, match="coincide"):
        rl.PointLight((0, 0, 0), 1, axis=(1, 0, 0), inner_deg=1e-9, outer_deg=2e-9).row()
    assert rl.light_rows([]).shape == (0, 16) and rl.light_rows([a, a]).shape == (2, 16) and rl.light_rows(a).shape == (1, 16)
    with pytest.raises(ValueError, match="PointLight"):
        rl.light_rows([a, (0, 0, 0)])
    with pytest.raises(RuntimeError, match="HIP device only"):
        rl.pack_lights([a], "cpu")
    with pytest.raises(ValueError, match="PointLight"):  # validation comes before the device
        rl.pack_lights([3.0], "cpu")


def test_argument_errors_come_before_any_device_call():
    from pano_nerf_amd import relight as rl
    H, W = 4, 6
    rgb, dep = torch.zeros(1, 3, H, W), torch.ones(1, 1, H, W)
    cam, pose = views.perspective_camera(H, W, fov_x_deg=60.0), np.eye(4)
    lt = [rl.PointLight((0, 1, 0), 1.0)]
    maps = torch.ones(1, 8, 16)
    ok = dict(rgb=rgb, depth=dep, normals=rgb, albedo=rgb, rays=(cam, pose), lights=lt, maps=maps)

    def call(**kw):
        return rl.relight(**{**ok, **kw})

    for kw, msg in ((dict(pcf=2), "pcf"), (dict(pcf=9), "pcf"), (dict(pcf=0), "pcf"), (dict(pcf=1.5), "pcf"),
                    (dict(map_kind="pinhole"), "map_kind"), (dict(bias_abs=-1e-3), "bias_abs"), (dict(bias_rel=-1.0), "bias_rel"),
                    (dict(bias_slope=-2.0), "bias_slope"), (dict(ambient=np.nan), "ambient"), (dict(normal_offset=np.inf), "normal_offset"),
                    (dict(bias_abs=1e39), "bias_abs"), (dict(albedo=torch.zeros(1, 3, H, W + 1)), "albedo"),
                    (dict(normals=torch.zeros(H * W, 3)), "normals"), (dict(depth=torch.ones(1, H, W)), "depth"),
                    (dict(rgb=torch.zeros(2, 3, H, W)), "image"), (dict(maps=torch.ones(2, 8, 16)), "1 lights but 2"),
                    (dict(maps=None), "need their shadow maps"), (dict(maps=torch.ones(1, 1, 16)), "at least 2 x 2"),
                    (dict(maps=torch.ones(1, 8, 16), map_kind="cube"), "6 W x W"), (dict(lights=[1.0]), "PointLight"),
                    (dict(lights=torch.zeros(1, 12)), "packed lights"), (dict(rays=cam), "rays must be"),
                    (dict(rays=(views.perspective_camera(H, W + 1, fov_x_deg=60.0), pose)), "camera is")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(RuntimeError, match="HIP device only"):  # everything is well-formed: the device is what is missing
        call()
    with pytest.raises(RuntimeError, match="HIP device only"):
        rl.light_visibility(torch.zeros(5, 3), lt, maps)
    with pytest.raises(ValueError, match="points"):
        rl.light_visibility(torch.zeros(5, 2), lt, maps)
    with pytest.raises(ValueError, match="normals"):
        rl.light_visibility(torch.zeros(5, 3), lt, maps, normals=torch.zeros(4, 3))
    with pytest.raises(ValueError, match="pcf"):
        rl.light_visibility(torch.zeros(5, 3), lt, maps, pcf=4)
    with pytest.raises(ValueError, match="kind"):
        rl.shadow_maps(None, lt, kind="fisheye")
    with pytest.raises(ValueError, match="base"):
        rl.relight_view(None, cam, pose, lt, base="albedo")
    with pytest.raises(ValueError, match="kinds"):
        rl.relight_path(None, cam, pose[None], lt, kinds=("depth",))
    with pytest.raises(ValueError, match="pcf"):
        rl.relight_view(None, cam, pose, lt, pcf=2)
