"""Relighting on the GPU: pn_relight against the fp64 restatement of tests/_relight_ref.py on every scene x map x pcf of its
analytic room, the edge rows, determinism, and the composition of shadow_maps / relight_view / relight_path from
render_view on a small random-initialised model.

Tolerances (from the number formats).  Both sides evaluate the header's formulas in fp64 on the same fp32 inputs and round
once.  Away from discrete decisions (the rows the restatement does not mark fragile: no tap within 1e-9 rho of its limit,
no bilinear fraction within 1e-9 of a floor) the two fp64 results differ by fp64 rounding noise only:
  visibility   a sum of at most 25 x 4 products of weights in [0, 1], divided by k^2: noise far below 2^-40, so the fp32
               roundings differ by at most one ulp of a value <= 1: 2^-23 absolute
  direct, rgb  the device's fp64 atan2 / sqrt / divide may differ from numpy's by an fp64 ulp, which can move a value across
               an fp32 rounding boundary: 2 ulp32(value), the allowance test_gpu_atlas makes
Each comparison prints the worst value it saw."""
import collections
import functools

import numpy as np
import pytest
import torch

import _relight_ref as ref

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def T(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).to(dev())


def N(x):
    return x.detach().cpu().numpy()


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def scene_rows(view):
    return ref.view_rows(view)


@functools.lru_cache(maxsize=None)
def scene_maps(m):
    return ref.shadow_maps(ref.light_rows(), *m)


RowRays = collections.namedtuple("RowRays", ["origins", "directions"])  # what relight reads of a Rays tuple


def run(rows, lights, maps, kind, pcf, use_normals=True, **kw):
    """pano_nerf_amd.relight.relight on numpy rows -> dict of numpy arrays"""
    from pano_nerf_amd import relight as rl
    rays = RowRays(T(rows["origins"]), T(rows["directions"]))
    out = rl.relight(T(rows["rgb"]), T(rows["depth"]), T(rows["normals"]) if use_normals else None, T(rows["albedo"]), rays,
                     T(lights).reshape(-1, 16), None if maps is None else T(maps), "pano" if kind == ref.MAP_PANO else "cube",
                     pcf=pcf, **kw)
    return out


def compare(got, want, tag):
    """the kernel's dict against the restatement's on the non-fragile rows; prints the worst errors"""
    keep = ~want["fragile"]
    share = float(keep.mean()) if keep.size else 1.0
    assert share >= 0.99, (tag, share)
    v_got, v_want = N(got["visibility"]).astype(np.float64), want["visibility"].astype(np.float32).astype(np.float64)
    assert v_got.shape == v_want.shape, (tag, v_got.shape, v_want.shape)
    ev = np.abs(v_got - v_want)[keep]
    worst_v = float(ev.max()) / 2.0 ** -23 if ev.size else 0.0
    msg = [f"visibility worst {worst_v:.2f} x 2^-23" if worst_v else "visibility worst 0 (exact)"]
    assert np.all(ev <= 2.0 ** -23), (tag, worst_v)
    for name, key in (("direct", "direct"), ("rgb", "out")):
        g = N(got[name]).astype(np.float64)
        w = want[key].astype(np.float32).astype(np.float64)
        assert g.shape == w.shape, (tag, name)
        err, u = np.abs(g - w)[keep], ulp32(w)[keep]
        worst = float((err / u).max()) if err.size else 0.0
        msg.append(f"{name} worst {worst:.2f} ulp" if worst else f"{name} worst 0 (exact)")
        assert np.all(err <= 2.0 * u), (tag, name, worst)
    print(f"{tag}: {int(keep.sum())} of {keep.size} rows compared; " + "; ".join(msg))


# ------------------------------------------------------------------------------------------- 1. kernel against reference
@pytest.mark.parametrize("pcf", ref.PCFS)
@pytest.mark.parametrize("m", ref.MAPS, ids=lambda m: f"{'pano' if m[0] == ref.MAP_PANO else 'cube'}{m[1]}x{m[2]}")
@pytest.mark.parametrize("view", ref.VIEWS)
def test_kernel_matches_the_restatement(view, m, pcf):
    rows, lights, maps = scene_rows(view), ref.light_rows(), scene_maps(m)
    want = ref.relight(rows, lights, maps, m[0], pcf)
    got = run(rows, lights, maps, m[0], pcf)
    compare(got, want, f"{view} map {m} pcf {pcf}")
    v = N(got["visibility"])
    assert (v == 0).any() and (v == 1).any() and ((v > 0) & (v < 1)).any()


def test_scalars_and_no_normals():
    """non-default ambient, offsets and biases (bias_slope = 0: the acne the slope term exists for), and normals = None"""
    rows, lights, m = scene_rows("pinhole"), ref.light_rows(), ref.MAPS[0]
    maps = scene_maps(m)
    for kw in (dict(ambient=0.35, normal_offset=0.0, bias_abs=0.0, bias_rel=0.0, bias_slope=0.0),
               dict(ambient=0.0, normal_offset=0.05, bias_abs=0.03, bias_rel=0.0, bias_slope=4.0),
               dict(ambient=-1.0, normal_offset=-0.01, bias_abs=0.0, bias_rel=0.1, bias_slope=0.5)):
        want = ref.relight(rows, lights, maps, m[0], 3, **kw)
        compare(run(rows, lights, maps, m[0], 3, **kw), want, f"scalars {kw}")
    want = ref.relight(rows, lights, maps, m[0], 3, use_normals=False)
    compare(run(rows, lights, maps, m[0], 3, use_normals=False), want, "no normals")
    # pcf = 7, the largest window, on the cube
    m = ref.MAPS[2]
    compare(run(rows, lights, scene_maps(m), m[0], 7), ref.relight(rows, lights, scene_maps(m), m[0], 7), "pcf 7 cube")


# ------------------------------------------------------------------------------------------------------ 2. edge cases
def test_edge_rows():
    rows = {k: v[:300].copy() for k, v in scene_rows("pano").items()}
    lights, m = ref.light_rows(), ref.MAPS[0]
    maps = scene_maps(m).copy()
    rows["depth"][:4] = (np.nan, 0.0, -1.0, np.inf)
    rows["normals"][4] = 0.0
    rows["normals"][5, 1] = np.nan
    rows["normals"][6] = (np.inf, 0.0, 0.0)
    rows["normals"][7] = 1e-20  # |n| below 1e-12
    maps[0, ::3, ::2] = np.nan  # no surface: lit
    maps[1, 1::3] = 0.0
    maps[2, :, ::4] = -2.0
    maps[2, 3, 5] = np.inf
    want = ref.relight(rows, lights, maps, m[0], 3, ambient=0.5)
    got = run(rows, lights, maps, m[0], 3, ambient=0.5)
    compare(got, want, "edge rows")
    assert not N(got["visibility"])[:8].any() and not N(got["direct"])[:8].any()
    assert bits_equal(got["rgb"][:8], (T(rows["rgb"][:8]).double() * 0.5).float())
    assert np.isfinite(N(got["rgb"])).all()
    # an empty map lights every facing row
    empty = np.full_like(maps, np.nan)
    empty[1], empty[2] = 0.0, -1.0
    v = N(run(rows, lights, empty, m[0], 5)["visibility"])
    w = ref.relight(rows, lights, empty, m[0], 5)
    lit = w["valid"][:, None] & (w["visibility"] > 0)
    assert lit.any() and np.all(v[lit] == 1.0) and np.all(v[~lit] == 0.0)


def test_light_inside_the_occluder_and_on_a_surface():
    from pano_nerf_amd import relight as rl
    rows = scene_rows("cube")
    inside = rl.light_rows([rl.PointLight(ref.SPHERE_C, 5.0, r_min=0.0)])
    for m in (ref.MAPS[0], ref.MAPS[2]):
        maps = np.full((1, m[1], m[2]), np.float32(ref.SPHERE_R))  # what the light sees: the inside of the sphere
        # bias_slope = 0: the limit is 1.02 r + 0.01 = 0.52 for every tap, and every wall is at least 0.9 from the centre
        want = ref.relight(rows, inside, maps, m[0], 3, bias_slope=0.0)
        got = run(rows, inside, maps, m[0], 3, bias_slope=0.0)
        compare(got, want, f"light inside the occluder, map {m}")
        walls = rows["sid"] != ref.SPHERE_ID
        assert walls.sum() > 100 and not N(got["visibility"])[walls].any() and not N(got["direct"])[walls].any()
        assert bits_equal(got["rgb"][T(walls, torch.bool)], T(rows["rgb"][walls]))
    # r2 = 0: X = o + t d is exactly the light's position
    R = 3
    one = dict(origins=np.zeros((R, 3), np.float32), directions=np.tile(np.float32([0.5, -1.0, 0.25]), (R, 1)),
               depth=np.float32([2.0, 2.0, 1.0]), normals=np.tile(np.float32([0, 1, 0]), (R, 1)),
               albedo=np.full((R, 3), 0.5, np.float32), rgb=np.float32([[0.1, 0.2, 0.3]] * R))
    at = rl.light_rows([rl.PointLight((1.0, -2.0, 0.5), 7.0, r_min=0.0), rl.PointLight((1.0, 0.0, 0.5), 2.0)])
    maps = np.full((2, 8, 16), 50.0, np.float32)
    got = run(one, at, maps, ref.MAP_PANO, 1)
    want = ref.relight(one, at, maps, ref.MAP_PANO, 1)
    compare(got, want, "light on the surface point")
    v = N(got["visibility"])
    assert v[0, 0] == 0 and v[1, 0] == 0 and v[0, 1] == 1 and np.isfinite(N(got["rgb"])).all()


def test_no_lights_no_rows_and_determinism():
    from pano_nerf_amd import relight as rl
    rows, lights, m = scene_rows("pinhole"), ref.light_rows(), ref.MAPS[1]
    maps = scene_maps(m)
    # L = 0 and ambient = 1: the input bits
    got = run(rows, lights[:0], None, m[0], 3)
    assert bits_equal(got["rgb"], T(rows["rgb"])) and tuple(got["visibility"].shape) == (len(rows["depth"]), 0)
    assert not N(got["direct"]).any()
    # R = 0
    none = {k: v[:0] for k, v in rows.items()}
    got = run(none, lights, maps, m[0], 3)
    assert tuple(got["rgb"].shape) == (0, 3) and tuple(got["visibility"].shape) == (0, 3)
    assert tuple(rl.light_visibility(torch.zeros(0, 3, device=dev()), T(lights), T(maps)).shape) == (0, 3)
    # twice the same bits; one call or split 100 / rest the same bits
    a, b = run(rows, lights, maps, m[0], 5), run(rows, lights, maps, m[0], 5)
    head, tail = ({k: v[:100] for k, v in rows.items()}, {k: v[100:] for k, v in rows.items()})
    h, t = run(head, lights, maps, m[0], 5), run(tail, lights, maps, m[0], 5)
    for k in ("rgb", "direct", "visibility"):
        assert bits_equal(a[k], b[k]), k
        assert bits_equal(a[k], torch.cat([h[k], t[k]])), k


def test_images_and_light_visibility():
    """[1, C, H, W] inputs with (camera, c2w) rays give the rows' result reshaped; light_visibility is relight's visibility"""
    from pano_nerf_amd import relight as rl, views
    cam, pose = ref.view_camera("pinhole"), ref.view_pose("pinhole")
    H, W = cam.h, cam.w
    rays = views.generate_camera_rays(cam, pose, device=dev())
    rows = dict(scene_rows("pinhole"))
    lights, m = ref.light_rows(), ref.MAPS[0]
    maps = scene_maps(m)
    img = lambda x, c: T(x).view(1, H, W, c).permute(0, 3, 1, 2)
    out = rl.relight(img(rows["rgb"], 3), img(rows["depth"], 1), img(rows["normals"], 3), img(rows["albedo"], 3), (cam, pose),
                     T(lights), T(maps), pcf=3)
    assert tuple(out["rgb"].shape) == (1, 3, H, W) and tuple(out["direct"].shape) == (1, 3, H, W)
    assert tuple(out["visibility"].shape) == (1, 3, H, W)
    flat = rl.relight(T(rows["rgb"]), T(rows["depth"]), T(rows["normals"]), T(rows["albedo"]), rays, T(lights), T(maps), pcf=3)
    for k, c in (("rgb", 3), ("direct", 3), ("visibility", 3)):
        assert bits_equal(out[k].permute(0, 2, 3, 1).reshape(-1, c), flat[k]), k
    # light_visibility: points as origins, zero directions, depth 1
    X = (rows["origins"].astype(np.float64) + rows["depth"][:, None].astype(np.float64) * rows["directions"]).astype(np.float32)
    pts = dict(rows, origins=X, directions=np.zeros_like(X), depth=np.ones(len(X), np.float32))
    for normals in (True, False):
        vis = rl.light_visibility(T(X), T(lights), T(maps), T(rows["normals"]) if normals else None, pcf=3)
        want = ref.relight(pts, lights, maps, m[0], 3, use_normals=normals)
        keep = ~want["fragile"]
        err = np.abs(N(vis).astype(np.float64) - want["visibility"].astype(np.float32))[keep]
        print(f"light_visibility normals={normals}: worst {err.max() / 2.0 ** -23:.2f} x 2^-23 over {int(keep.sum())} rows")
        assert keep.mean() >= 0.99 and np.all(err <= 2.0 ** -23)


def test_error_codes():
    from pano_nerf_amd import _lib
    lib = _lib.load()
    R, L = 8, 1
    f = lambda *s: torch.ones(*s, device=dev())
    o, d, t, n, a, c, lt, mp = f(R, 3), f(R, 3), f(R), f(R, 3), f(R, 3), f(R, 3), torch.zeros(L, 16, device=dev()), f(L, 8, 16)
    out, direct, vis = f(R, 3), f(R, 3), f(R, L)
    st = _lib.stream(dev())

    def call(**kw):
        arg = dict(R=R, o=o, d=d, t=t, n=n, a=a, c=c, L=L, lt=lt, kind=0, Hm=8, Wm=16, mp=mp, amb=1.0, off=0.02, ba=0.01,
                   br=0.02, bs=2.0, k=3, out=out, direct=direct, vis=vis)
        arg.update(kw)
        p = lambda x: None if x is None else x.data_ptr()
        return lib.pn_relight(arg["R"], p(arg["o"]), p(arg["d"]), p(arg["t"]), p(arg["n"]), p(arg["a"]), p(arg["c"]), arg["L"],
                              p(arg["lt"]), arg["kind"], arg["Hm"], arg["Wm"], p(arg["mp"]), arg["amb"], arg["off"], arg["ba"],
                              arg["br"], arg["bs"], arg["k"], p(arg["out"]), p(arg["direct"]), p(arg["vis"]), st)

    OK, SHAPE, UNSUPPORTED, NULL = 0, -1, -2, -3
    assert call() == OK
    for kw in (dict(R=-1), dict(L=-1), dict(k=2), dict(k=0), dict(k=9), dict(k=-3), dict(Hm=1), dict(Wm=1),
               dict(kind=2, Hm=8, Wm=16), dict(amb=float("nan")), dict(off=float("inf")), dict(ba=-0.5), dict(br=-1e-6),
               dict(bs=-1.0), dict(bs=float("nan"))):
        assert call(**kw) == SHAPE, kw
    for kind in (1, 3, 4, 7, -1):
        assert call(kind=kind) == UNSUPPORTED, kind
    for kw in (dict(o=None), dict(d=None), dict(t=None), dict(lt=None), dict(mp=None), dict(a=None), dict(c=None),
               dict(a=None, c=None), dict(a=None, out=None), dict(c=None, direct=None)):
        assert call(**kw) == NULL, kw
    assert call(n=None) == OK and call(a=None, c=None, out=None, direct=None) == OK
    assert call(out=None) == OK and call(direct=None, vis=None) == OK
    assert call(L=0, lt=None, mp=None) == OK and call(R=0, o=None, d=None, t=None) == OK
    assert call(kind=2, Hm=12, Wm=2, mp=f(1, 12, 2)) == OK
    torch.cuda.synchronize()
    assert b"shape" in lib.pn_strerror(SHAPE).lower() and lib.pn_strerror(UNSUPPORTED).decode().startswith("unsupported")


# ------------------------------------------------------------------------------------------------------ 3. composition
@functools.lru_cache(maxsize=None)
def model():
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    m = pn.PanoMipNeRF(num_samples=16, rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    m.mlp.load_state_dict(orc.init_params(4, 5))
    return m.to(dev())


def scene_lights():
    from pano_nerf_amd import relight as rl
    return [rl.PointLight((0.3, 0.4, -0.2), (3.0, 2.0, 1.0)),
            rl.PointLight((-0.4, 0.5, 0.3), 2.0, axis=(0.3, -1.0, -0.2), inner_deg=25.0, outer_deg=50.0)]


def pose_at(p):
    m = np.eye(4)
    m[:3, 3] = p
    return m


def test_shadow_maps_are_render_view_depth():
    from pano_nerf_amd import relight as rl, views
    lights = scene_lights()
    rows = rl.light_rows(lights)
    maps = rl.shadow_maps(model(), lights, 8, 16)
    cube = rl.shadow_maps(model(), T(rows[:, :3]), width=4, kind="cube", chunk_rays=50)
    assert tuple(maps.shape) == (2, 8, 16) and tuple(cube.shape) == (2, 24, 4)
    for i in range(2):
        p = rows[i, :3].astype(np.float64)
        want = views.render_view(model(), views.pano_camera(8, 16), pose_at(p), outputs=("depth",))["fine_dep"]
        assert bits_equal(maps[i], want[0, 0]), i
        want = views.render_view(model(), views.cubemap_camera(4), pose_at(p), outputs=("depth",))["fine_dep"]
        assert bits_equal(cube[i], want[0, 0]), i
    assert bool(torch.isfinite(maps).all()) and bool(torch.isfinite(cube).all())
    assert tuple(rl.shadow_maps(model(), [], 8, 16).shape) == (0, 8, 16)
    with pytest.raises(RuntimeError, match="HIP device only"):
        rl.shadow_maps(model(), torch.zeros(1, 3), 8, 16)


def test_relight_view_and_path_are_the_composition():
    import pano_nerf_amd as pn
    from pano_nerf_amd import relight as rl, views
    H, W = 12, 16
    env = pn.generate_lit_rays(10, 0.01)
    cam = views.perspective_camera(H, W, fov_x_deg=70.0)
    poses = np.stack([views.look_at((0.2, 0.1, 1.5), (0, 0, 0)), views.look_at((-0.6, 0.3, 1.2), (0, 0, 0))])
    lights = scene_lights()
    kw = dict(ambient=0.8, pcf=3, bias_slope=1.5)
    maps = rl.shadow_maps(model(), lights, 8, 16)
    for base in ("fine_rgb", "surface_rgb"):
        got = rl.relight_view(model(), cam, poses[0], lights, env, base=base, map_size=(8, 16), **kw)
        view = views.render_view(model(), cam, poses[0], env, outputs=("rgb", "depth", "normal", "albedo", "surface"))
        hand = rl.relight(view[base], view["fine_dep"], view["fine_nor"], view["albedo"], (cam, poses[0]), lights, maps, **kw)
        assert bits_equal(got["relit_rgb"], hand["rgb"]) and bits_equal(got["direct"], hand["direct"]), base
        assert bits_equal(got["visibility"], hand["visibility"]), base
        for k in ("fine_rgb", "fine_dep", "fine_nor", "albedo"):
            assert bits_equal(got[k], view[k]), (base, k)
        assert tuple(got["visibility"].shape) == (1, 2, H, W) and bool(torch.isfinite(got["relit_rgb"]).all())
    assert float(got["direct"].max()) > 0  # the lamps reach something
    given = rl.relight_view(model(), cam, poses[0], lights, env, maps=maps, **kw)
    assert bits_equal(given["relit_rgb"], rl.relight_view(model(), cam, poses[0], lights, env, map_size=(8, 16), **kw)["relit_rgb"])
    # no lights: the rendered image itself
    bare = rl.relight_view(model(), cam, poses[0], [], env)
    assert bits_equal(bare["relit_rgb"], bare["fine_rgb"]) and tuple(bare["visibility"].shape) == (1, 0, H, W)
    assert bits_equal(bare["fine_rgb"], views.render_view(model(), cam, poses[0], env, outputs=("rgb",))["fine_rgb"])
    # the path: frames of relight_view, the maps rendered once
    kinds = ("ldr", "hdr", "direct")
    fr = rl.relight_path(model(), cam, poses, lights, env, map_size=(8, 16), kinds=kinds, exposure=0.5, **kw)
    assert sorted(fr) == sorted(kinds)
    for i in range(2):
        v = rl.relight_view(model(), cam, poses[i], lights, env, maps=maps, **kw)
        assert bits_equal(fr["hdr"][i], v["relit_rgb"][0].permute(1, 2, 0)), i
        assert bits_equal(fr["ldr"][i], views.to_frame(v["relit_rgb"], "ldr", exposure=0.5)), i
        assert bits_equal(fr["direct"][i], views.to_frame(v["direct"], "ldr", exposure=0.5)), i
    with pytest.raises(ValueError, match="env_rays"):
        rl.relight_view(model(), cam, poses[0], lights)


def test_relight_path_writes_files(tmp_path):
    import pano_nerf_amd as pn
    from pano_nerf_amd import io_exr, relight as rl, views
    env = pn.generate_lit_rays(10, 0.01)
    cam = views.pano_camera(8, 16)
    poses = np.stack([pose_at((0.0, 0.0, 0.0)), pose_at((0.1, 0.0, -0.1))])
    lights = scene_lights()
    fr = rl.relight_path(model(), cam, poses, lights, env, map_size=(8, 16), kinds=("ldr", "hdr"))
    res = rl.relight_path(model(), cam, poses, lights, env, map_size=(8, 16), kinds=("ldr", "hdr"), out_dir=str(tmp_path))
    assert res == {}
    for i in range(2):
        assert np.array_equal(io_exr.read_exr(str(tmp_path / "hdr" / f"{i:05d}.exr")), N(fr["hdr"][i]))
        assert (tmp_path / "ldr" / f"{i:05d}.png").stat().st_size > 0
