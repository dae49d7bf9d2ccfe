"""views.fill_holes / pn_fill_holes and views.blend_warps / pn_warp_blend on the GPU against the numpy reference
(tests/_fill_ref.py, written from include/panonerf_hip.h and audited by test_fill_cpu.py), bit for bit: every operation of
the rule is a correctly rounded fp32 +, * or / in a stated order, so there is no tolerance.  Where the reference is NaN the
kernel need only be NaN.  And views.render_path_warped with blend / inpaint against the same calls composed by hand.

The shapes are the smallest at which the kernels can go wrong: 1 x 1 (no level above the frame), 1 x 2, odd sizes (a level
whose last row or column has no sibling), 8 x 16 (every level even), a panorama (columns wrap at every level), a cube
strip (six images per frame), a fisheye (a domain), and 66 x 70, the smallest frame whose first level is too large for the
one-workgroup kernel of the small levels, so that the per-level kernels run too, on more than one workgroup."""
import numpy as np
import pytest
import torch

import _fill_ref as fr

pytestmark = pytest.mark.gpu

F = np.float32
DENSITIES = [0.0, 0.02, 0.5, 0.98, 1.0]
BAD_SHAPE, NULL = -1, -3


def dev():
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def same_bits(got, want, what):
    """bit for bit, except that where the reference is NaN the result need only be NaN"""
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), what
    bad = (bits(got) != bits(want)) & ~nan
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def frames():
    """(name, H, W, camera) of every frame kind"""
    from pano_nerf_amd import views
    out = [(f"{h}x{w}", h, w, None) for h, w in fr.SIZES]
    out += [("pano16x32", 16, 32, views.pano_camera(16, 32)), ("cube24x4", 24, 4, views.cubemap_camera(4)),
            ("fisheye9x9", 9, 9, views.fisheye_camera(9, 9, fov_deg=150.0)), ("pinhole7x10", 7, 10,
                                                                           views.perspective_camera(7, 10, fov_x_deg=60.0))]
    return out


def make(H, W, density, N, C, seed=0):
    img, dep, known = fr.scene(H, W, density, seed, N, C)
    if density == 0.0:
        known[:] = False
    if density == 1.0:
        known[:] = True
    flat = dep.reshape(-1)  # depths that are no depths make a covered pixel unknown
    for i, v in enumerate((np.nan, 0.0, np.inf, -1.0)):
        if flat.size > 7 * i + 3:
            flat[7 * i + 3] = v
    return img, dep, known


def reference(img, dep, known, cam, r, levels):
    """the reference through the camera conventions of views.fill_holes"""
    from pano_nerf_amd import views
    N, C, H, W = img.shape
    if isinstance(cam, views.CubeCamera):
        faces = img.reshape(N, C, 6, W, W).transpose(0, 2, 1, 3, 4).reshape(6 * N, C, W, W)
        o, d, f = fr.fill_holes(faces, None if dep is None else dep.reshape(6 * N, W, W),
                                None if known is None else known.reshape(6 * N, W, W), None, False, r, levels)
        o = o.reshape(N, 6, C, W, W).transpose(0, 2, 1, 3, 4).reshape(N, C, H, W)
        return o, None if d is None else d.reshape(N, H, W), f.reshape(N, H, W)
    domain = views.camera_mask(cam) if isinstance(cam, views.FisheyeCamera) else None
    return fr.fill_holes(img, dep, known, domain, isinstance(cam, views.PanoCamera), r, levels)


def run_and_compare(img, dep, known, cam, r, levels, what):
    from pano_nerf_amd import views
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())  # noqa: E731
    cov = None if known is None else known.astype(F)
    got = views.fill_holes(t(img), t(dep), t(cov), cam, r, levels)
    want_i, want_d, want_f = reference(img, dep, known, cam, r, levels)
    assert sorted(got) == (["depth", "filled", "image"] if dep is not None else ["filled", "image"]), what
    assert got["filled"].dtype == torch.bool and np.array_equal(got["filled"].cpu().numpy(), want_f), what
    same_bits(got["image"].cpu().numpy(), want_i, what)
    if dep is not None:
        assert got["depth"].shape == (img.shape[0], 1) + img.shape[2:]
        same_bits(got["depth"].cpu().numpy()[:, 0], want_d, what)
    return got, (want_i, want_d, want_f)


@pytest.mark.parametrize("frame", frames(), ids=lambda f: f[0])
def test_fill_holes_matches_the_reference(frame):
    """every frame kind at every density, with and without a depth; C, N and r rotate through their values"""
    name, H, W, cam = frame
    i = 0
    for density in DENSITIES:
        for with_depth in (False, True):
            C, N, r = (1, 3, 4)[i % 3], (1, 3)[i % 2], (0.05, 0.0, 0.5)[(i // 2) % 3]
            i += 1
            img, dep, known = make(H, W, density, N, C, seed=i)
            what = (name, density, with_depth, C, N, r)
            got, (_, _, want_f) = run_and_compare(img, dep if with_depth else None, known, cam, r, None, what)
            if density == 0.0:  # nothing known: nothing changes
                assert not want_f.any() and np.array_equal(bits(got["image"].cpu().numpy()), bits(img)), what
            if density == 1.0 and not with_depth:  # everything known: the identity
                assert not want_f.any() and np.array_equal(bits(got["image"].cpu().numpy()), bits(img)), what


@pytest.mark.parametrize("levels", [None, 0, 2])
@pytest.mark.parametrize("r", [0.0, 0.05, 0.5])
def test_ratio_levels_channels_images(r, levels):
    from pano_nerf_amd import views
    for H, W, cam in ((7, 10, None), (16, 32, views.pano_camera(16, 32))):
        for C in (1, 3, 4):
            for N in (1, 3):
                img, dep, known = make(H, W, 0.3, N, C, seed=C + N)
                img[0, 0, 0, 0], known[0, 0, 0] = np.nan, True  # a NaN colour spreads into what it fills
                got, (_, _, want_f) = run_and_compare(img, dep, known, cam, r, levels, (H, W, C, N, r, levels))
                if levels == 0:
                    assert not want_f.any()
                if levels is None:
                    assert bool(torch.isfinite(got["depth"]).all())  # complete: what to_frame needs


@pytest.mark.parametrize("C,levels", [(3, None), (3, 2), (3, 1), (40, None)])
def test_where_the_small_levels_share_one_launch(C, levels):
    """Levels of at most 1024 texels whose planes fit into 48 KB of LDS run in one workgroup per image; larger ones get a
    launch each.  66 x 70: level 1 (33 x 35 = 1155 texels) is too large and level 2 (17 x 18) is not; with 40 channels
    level 2 does not fit either; capped levels end below, at and above that border.  (Every other frame of this file is
    small enough for the one launch to reach down to the frame itself.)"""
    from pano_nerf_amd import views
    img, dep, known = make(66, 70, 0.02, 2, C)
    run_and_compare(img, dep, known, views.pano_camera(66, 70), 0.05, levels, (C, levels))


def test_none_arguments_noncontiguous_inputs_and_repeats():
    from pano_nerf_amd import views
    img, dep, known = make(7, 10, 0.5, 3, 3)
    x, z, cov = (torch.from_numpy(a).to(dev()) for a in (img, dep, known.astype(F)))
    first, _ = run_and_compare(img, dep, known, None, 0.05, None, "plain")
    # the same frames held as [N, H, W, C], every second row of a taller depth, coverage as [N, 1, H, W] and as bool
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    tall = torch.zeros(3, 14, 10, device=dev())
    tall[:, ::2] = z
    before = nhwc.clone()
    for c in (cov[:, None], cov > 0):
        again = views.fill_holes(nhwc.permute(0, 3, 1, 2), tall[:, ::2], c, None)
        for k in first:
            assert torch.equal(again[k].view(torch.uint8), first[k].view(torch.uint8)), k
    assert torch.equal(nhwc.view(torch.int32), before.view(torch.int32))  # the inputs are untouched
    assert torch.equal(tall[:, ::2].contiguous().view(torch.int32), z.view(torch.int32))
    # no coverage: the depth alone says what is known; no depth, no coverage: the identity
    run_and_compare(img, dep, None, None, 0.05, None, "no coverage")
    got, _ = run_and_compare(img, None, None, None, 0.05, None, "nothing unknown")
    assert not bool(got["filled"].any())
    # one frame without batch dimensions
    one = views.fill_holes(x[0], z[0], cov[0])
    assert one["image"].shape == (1, 3, 7, 10) and one["depth"].shape == (1, 1, 7, 10) and one["filled"].shape == (1, 7, 10)
    assert torch.equal(one["image"][0].view(torch.int32), first["image"][0].view(torch.int32))


def test_background_scene_and_wrap_scene():
    """the audited scenes of test_fill_cpu.py, on the device"""
    from pano_nerf_amd import views
    img, dep, known = fr.background_scene()
    got, _ = run_and_compare(img, dep, known, None, 0.05, None, "background")
    hole = torch.from_numpy(~known[0]).to(dev())
    assert bool((got["image"][0, 0][hole] == 0.25).all()) and bool((got["depth"][0, 0][hole] == 4.0).all())
    blind, _ = run_and_compare(img, None, known, None, 0.05, None, "blind")
    assert bool((blind["image"][0, 0][hole] > 0.25).all())
    strip = np.zeros((1, 1, 4, 16), F)
    strip[..., 8:] = 1.0
    k = np.ones((1, 4, 16), bool)
    k[..., :2] = False
    w, _ = run_and_compare(strip, None, k, views.pano_camera(4, 16), 0.05, None, "wrap")
    p, _ = run_and_compare(strip, None, k, None, 0.05, None, "no wrap")
    assert bool((w["image"][0, 0, :, 0] == 0.4375).all()) and bool((p["image"][0, 0, :, 0] == 0).all())


def test_an_empty_cube_face_stays_a_hole():
    from pano_nerf_amd import views
    S = 4
    img, dep, known = make(6 * S, S, 0.5, 2, 3)
    known[0, 2 * S:3 * S] = False  # face +y of the first strip: nothing known
    got, _ = run_and_compare(img, dep, known, views.cubemap_camera(S), 0.05, None, "cube")
    f = got["filled"].cpu().numpy()
    assert not f[0, 2 * S:3 * S].any()
    assert np.array_equal(bits(got["image"].cpu().numpy()[0, :, 2 * S:3 * S]), bits(img[0, :, 2 * S:3 * S]))
    assert f[0, S:2 * S].any() and f[0, 3 * S:4 * S].any()  # its neighbours in the strip are filled


def call_fill(lib, x, z, known, domain, filled, work, N=None, C=None, H=None, W=None, wrap=0, r=0.05, levels=32, floats=None):
    n, c, h, w = x.shape
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return lib.pn_fill_holes(n if N is None else N, c if C is None else C, h if H is None else H, w if W is None else W,
                             p(x), p(z), p(known), p(domain), wrap, r, levels, p(filled), p(work),
                             (0 if work is None else work.numel()) if floats is None else floats, None)


def test_c_entry_point_and_error_codes():
    from pano_nerf_amd import views, _lib
    lib = _lib.load()
    assert lib.pn_abi_version() == 2
    N, C, H, W = 3, 2, 9, 9
    img, dep, known = make(H, W, 0.4, N, C)
    yy, xx = np.mgrid[:H, :W]
    dom = (yy - 4) ** 2 + (xx - 4) ** 2 <= 17
    floats = lib.pn_fill_holes_work_floats(N, C, H, W, 32)
    assert floats == N * (C + 1) * sum(h * w for h, w in fr.level_sizes(H, W)[1:])
    assert lib.pn_fill_holes_work_floats(N, C, H, W, 2) == N * (C + 1) * (25 + 9) and lib.pn_fill_holes_work_floats(N, C, H, W, 0) == 0
    x, z, k = (torch.from_numpy(a).to(dev()) for a in (img, dep, known.astype(F)))
    d = torch.from_numpy(dom.astype(np.uint8)).to(dev())
    filled = torch.full((N, H, W), 7, dtype=torch.uint8, device=dev())
    work = torch.empty(floats, device=dev())
    # every refusal happens before a launch: the buffers keep their bits
    x0, z0 = x.clone(), z.clone()
    args = (lib, x, z, k, d, filled, work)
    for bad in (dict(N=0), dict(C=0), dict(H=0), dict(W=-1), dict(r=1.0), dict(r=-0.01), dict(r=float("nan")),
                dict(r=float("inf")), dict(levels=-1), dict(floats=floats - 1), dict(N=1 << 20, H=1 << 10, W=1 << 10)):
        assert call_fill(*args, **bad) == BAD_SHAPE, bad
    assert lib.pn_fill_holes(N, C, H, W, None, z.data_ptr(), k.data_ptr(), d.data_ptr(), 0, 0.05, 32, filled.data_ptr(),
                             work.data_ptr(), floats, None) == NULL
    assert lib.pn_fill_holes(N, C, H, W, x.data_ptr(), z.data_ptr(), k.data_ptr(), d.data_ptr(), 0, 0.05, 32, None,
                             work.data_ptr(), floats, None) == NULL
    assert lib.pn_fill_holes(N, C, H, W, x.data_ptr(), z.data_ptr(), k.data_ptr(), d.data_ptr(), 0, 0.05, 32, filled.data_ptr(),
                             None, floats, None) == NULL
    for n_, c_, h_, w_, l_ in ((0, 1, 4, 4, 1), (1, 0, 4, 4, 1), (1, 1, 0, 4, 1), (1, 1, 4, 0, 1), (1, 1, 4, 4, -1)):
        assert lib.pn_fill_holes_work_floats(n_, c_, h_, w_, l_) == BAD_SHAPE
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int32), x0.view(torch.int32)) and torch.equal(z.view(torch.int32), z0.view(torch.int32))
    assert bool((filled == 7).all())
    # the call itself, in place, with a domain and wrapping columns
    assert call_fill(*args, wrap=1) == 0
    want_i, want_d, want_f = fr.fill_holes(img, dep, known, dom, True, 0.05, None)
    same_bits(x.cpu().numpy(), want_i, "image")
    same_bits(z.cpu().numpy(), want_d, "depth")
    assert np.array_equal(filled.cpu().numpy(), want_f.astype(np.uint8))
    # blend
    im = torch.zeros(2, 1, 3, 6, 8, device=dev())
    dp = torch.ones(2, 1, 6, 8, device=dev())
    wt = torch.ones(2, 1, device=dev())
    o, od, oc = torch.full((1, 3, 6, 8), 5.0, device=dev()), torch.full((1, 6, 8), 5.0, device=dev()), torch.full((1, 6, 8), 5.0, device=dev())

    def blend(S=2, D=1, C=3, H=6, W=8, r=0.05, images=im, out=o):
        return lib.pn_warp_blend(S, D, C, H, W, None if images is None else images.data_ptr(), dp.data_ptr(), wt.data_ptr(), r,
                                 0.0, None if out is None else out.data_ptr(), od.data_ptr(), oc.data_ptr(), None)

    for bad in (dict(S=0), dict(D=0), dict(C=0), dict(H=0), dict(W=0), dict(r=1.0), dict(r=-1.0), dict(r=float("nan")),
                dict(S=1 << 12, H=1 << 10, W=1 << 10)):
        assert blend(**bad) == BAD_SHAPE, bad
    assert blend(images=None) == NULL and blend(out=None) == NULL
    torch.cuda.synchronize()
    assert bool((o == 5).all()) and bool((od == 5).all()) and bool((oc == 5).all())
    assert blend() == 0
    assert bool((o == 0).all()) and bool((od == 1).all()) and bool((oc == 1).all())


def test_python_error_paths():
    from pano_nerf_amd import views
    x = torch.zeros(1, 3, 8, 16, device=dev())
    z = torch.ones(1, 8, 16, device=dev())
    ok = dict(image=x, depth=z, coverage=z, camera=views.pano_camera(8, 16))
    views.fill_holes(**ok)
    for change, exc in ((dict(camera=views.stereo_pano_camera(8, 16, 0.06, "left")), ValueError),
                        (dict(camera=views.pano_camera(8, 18)), ValueError), (dict(depth_ratio=1.0), ValueError),
                        (dict(depth_ratio=-0.1), ValueError), (dict(depth_ratio=float("nan")), ValueError),
                        (dict(levels=-1), ValueError), (dict(levels=1.5), ValueError),
                        (dict(depth=torch.ones(1, 8, 15, device=dev())), ValueError),
                        (dict(coverage=torch.ones(2, 8, 16, device=dev())), ValueError),
                        (dict(image=torch.zeros(8, 16, device=dev())), ValueError),
                        (dict(image=x.cpu()), RuntimeError), (dict(depth=z.cpu()), RuntimeError)):
        with pytest.raises(exc):
            views.fill_holes(**{**ok, **change})
    im = torch.zeros(2, 1, 3, 6, 8, device=dev())
    dp = torch.ones(2, 1, 6, 8, device=dev())
    ok = dict(images=im, depths=dp, weights=[1.0, 2.0])
    views.blend_warps(**ok)
    for change, exc in ((dict(weights=[1.0, 0.0]), ValueError), (dict(weights=[1.0, -1.0]), ValueError),
                        (dict(weights=[1.0, float("inf")]), ValueError), (dict(weights=[1.0, float("nan")]), ValueError),
                        (dict(weights=[1.0]), ValueError), (dict(weights=[[1.0, 1.0]]), ValueError),
                        (dict(depths=dp[:, :, :5]), ValueError), (dict(images=im[0]), ValueError),
                        (dict(depth_ratio=1.0), ValueError), (dict(images=im.cpu()), RuntimeError)):
        with pytest.raises(exc):
            views.blend_warps(**{**ok, **change})


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_blend_warps_matches_the_reference(S, D):
    from pano_nerf_amd import views
    C, H, W = 3, 6, 8
    rng = np.random.default_rng(10 * S + D)
    img = rng.uniform(0, 1, (S, D, C, H, W)).astype(F)
    # depths near 2 so that layers are kept and occluded at r = 0.05, with what is no depth mixed in
    dep = (2.0 * (1.0 + rng.uniform(-0.06, 0.06, (S, D, H, W)))).astype(F)
    dep[rng.uniform(0, 1, dep.shape) < 0.3] = np.nan
    dep[rng.uniform(0, 1, dep.shape) < 0.1] = 0.0
    dep[rng.uniform(0, 1, dep.shape) < 0.1] = np.inf
    dep[rng.uniform(0, 1, dep.shape) < 0.05] = -1.0
    dep[:, :, 0, 0], dep[:, :, 0, 1] = 2.0, np.nan  # every layer on one surface; no layer at all
    img[0, 0, 1, 2, 3] = np.nan
    w = rng.uniform(0.1, 1.0, (S, D))
    for r in (0.05, 0.0):
        for weights in (w, w[:, 0]):
            got = views.blend_warps(torch.from_numpy(img).to(dev()), torch.from_numpy(dep).to(dev())[:, :, None], weights, r, -3.0)
            want_i, want_d, want_c = fr.blend(img, dep, weights, r, -3.0)
            assert want_c.min() == 0 and want_c.max() == 1
            same_bits(got["image"].cpu().numpy(), want_i, ("image", r))
            assert got["depth"].shape == (D, 1, H, W)
            same_bits(got["depth"].cpu().numpy()[:, 0], want_d, ("depth", r))
            assert np.array_equal(got["coverage"].cpu().numpy(), want_c)
    if S == 1:  # a single source costs nothing: its bits where it counts
        ok = want_c[0] > 0
        assert np.array_equal(bits(got["image"].cpu().numpy()[0][:, ok]), bits(img[0, 0][:, ok]))


# ------------------------------------------------------------------------------------------------ render_path_warped
def make_model():
    """the tiny model of tests/test_gpu_warp.py"""
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    model = pn.PanoMipNeRF(num_samples=16, rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    model.mlp.load_state_dict(orc.init_params(4, 5))
    model = model.to(dev())
    model.mlp_mode = "fused_f16x2"
    return model


def same(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype == torch.uint8:
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_render_path_warped_blend_and_inpaint():
    from pano_nerf_amd import views
    model = make_model()
    H, W, n = 12, 16, 5
    cam = views.perspective_camera(H, W, fov_x_deg=60.0)
    poses = np.stack([views.look_at([0.15 * i - 0.3, 0.05 * i, 2.0 - 0.1 * i], [0, 0, 0]) for i in range(n)])
    kinds = ("ldr", "depth", "hdr")
    kw = dict(kinds=kinds, near=0.0, far=10.0, exposure=0.5, max_splat=1, fill=0.125)
    full = views.render_path(model, cam, poses, kinds=kinds, near=0.0, far=10.0, exposure=0.5)
    keys = {j: views.render_view(model, cam, poses[j], outputs=("rgb", "depth")) for j in (0, 2, 4)}
    plain = views.render_path_warped(model, cam, poses, 2, **kw)
    holes = 0
    for blend, inpaint in ((True, False), (False, True), (True, True)):
        got = views.render_path_warped(model, cam, poses, 2, blend=blend, inpaint=inpaint, depth_ratio=0.1, **kw)
        assert sorted(got) == sorted(kinds + ("coverage",))
        for i in (0, 2, 4):  # rendered poses are never touched
            for k in kinds:
                assert same(got[k][i], full[k][i]), (k, i)
            assert bool((got["coverage"][i] == 1).all())
        for i in (1, 3):
            a, b = keys[i - 1], keys[i + 1]
            if blend:
                ws = [views.warp_view(v["fine_rgb"], v["fine_dep"], cam, poses[j], cam, poses[i], max_splat=1, fill=0.125)
                      for v, j in ((a, i - 1), (b, i + 1))]
                w = views.blend_warps(torch.stack([ws[0]["image"], ws[1]["image"]]), torch.stack([ws[0]["depth"], ws[1]["depth"]]),
                                      [0.5, 0.5], 0.1, 0.125)
            else:
                w = views.warp_view(torch.cat([a["fine_rgb"], b["fine_rgb"]]), torch.cat([a["fine_dep"], b["fine_dep"]]), cam,
                                    poses[[i - 1, i + 1]], cam, poses[i], max_splat=1, fill=0.125)
            cov = w["coverage"]
            holes += int((cov == 0).sum())
            if inpaint:
                f = views.fill_holes(w["image"], w["depth"], cov, cam, 0.1)
                assert bool(torch.equal(f["filled"], cov == 0)) and bool(torch.isfinite(f["depth"]).all())
                w = {**w, **f}
            assert same(got["hdr"][i], w["image"][0].permute(1, 2, 0)), (blend, inpaint, i)
            assert same(got["ldr"][i], views.to_frame(w["image"], "ldr", exposure=0.5)), (blend, inpaint, i)
            assert same(got["depth"][i], views.to_frame(w["depth"], "depth", 0.0, 10.0)), (blend, inpaint, i)
            assert same(got["coverage"][i], cov[0]), (blend, inpaint, i)
            if inpaint:
                assert int(got["depth"][i].max()) > 0  # a complete depth: no black frame
        if inpaint and not blend:  # coverage is the warp's own, the record of what was invented
            assert same(got["coverage"], plain["coverage"])
    assert holes > 0  # the warps of this path do leave holes, so the fill had work to do
    for i in (1, 3):  # and without inpaint a hole makes the depth frame black
        assert bool((plain["coverage"][i] == 1).all()) or int(plain["depth"][i].max()) == 0
