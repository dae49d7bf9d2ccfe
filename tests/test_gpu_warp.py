"""views.warp_view on the GPU against the numpy reference (tests/_warp_ref.py, written from include/panonerf_hip.h), on
the smallest scenes at which the kernels can still go wrong (the list _warp_ref.SCENES, audited by test_warp_cpu.py), and
views.render_path_warped against render_path / render_view / warp_view composed by hand.

The margin.  A forward warp makes discrete decisions (which pixels a splat covers, whether a point projects at all) from
fp32 positions, so the index map is compared through candidate sets made at a margin of m = 1e-3 px.  m is ten times an
estimate, not a measurement: a few fp32 roundings at |X| <= 4.5 give about 1e-6 absolute, which over rho >= 0.5 is 2e-6
rad, i.e. <= 1e-4 px at these focal lengths and widths (the largest: 32 px / 2 pi = 5 px per radian for the panorama,
8.6 for the fisheye, 24 for the 60 degree pinhole).  Where the reference itself is undecided at that margin (a "fragile"
pixel) only the candidate sets are checked; everywhere else the index must be the fp64 reference's.  A non-fragile
mismatch is a finding to explain, not a reason to widen m."""
import numpy as np
import pytest
import torch

import _cameras_ref as cr
import _warp_ref as wr

pytestmark = pytest.mark.gpu

CASES = [(s, k) for s in wr.SCENES for k in wr.SPLATS]
IDS = [f"{s['name']}-k{k}" for s, k in CASES]
FILL = -3.0
_RUNS = {}


def dev():
    return torch.device("cuda:0")


def _image(scene):
    rng = np.random.default_rng(17)
    img = rng.uniform(0, 1, (2, 3, scene["src"].h, scene["src"].w)).astype(np.float32)
    img[1, 2, 3, 4] = np.nan  # NaN is a colour like any other
    return img


def run(scene, max_splat):
    """warp_view of a scene, once: host copies of its outputs (read-only, shared among the tests)"""
    from pano_nerf_amd import views
    key = (scene["name"], max_splat)
    if key not in _RUNS:
        img = torch.from_numpy(_image(scene)).to(dev())
        dep = torch.from_numpy(scene["depth"]).to(dev())
        out = views.warp_view(img, dep, scene["src"], scene["src_c2ws"], scene["dst"], scene["dst_c2ws"], max_splat=max_splat,
                              fill=FILL)
        torch.cuda.synchronize()
        _RUNS[key] = {k: v.cpu().numpy() for k, v in out.items()}
    return _RUNS[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("scene,max_splat", CASES, ids=IDS)
def test_index_lies_in_the_candidate_sets(scene, max_splat):
    """pointwise, every destination pixel: the kernel's index is in the widened set, or -1 where the shrunk set is empty;
    and no member of the shrunk set is nearer than the chosen point by more than 1e-5 relative"""
    res = wr.reference(scene, max_splat)
    got = run(scene, max_splat)["index"]
    D, H, W = got.shape
    assert got.dtype == np.int64 and (D, H, W) == (3, scene["dst"].h, scene["dst"].w)
    for d in range(D):
        g = got[d].reshape(-1)
        wide, shrunk, rho = res["wide"][d], res["shrunk"][d], res["rho"][d].astype(np.float64)
        hole = g < 0
        assert (g[hole] == -1).all()
        assert not shrunk[hole].any(), (d, np.where(shrunk[hole].any(-1))[0][:5])
        pix = np.where(~hole)[0]
        assert (g[pix] < wide.shape[1]).all() and wide[pix, g[pix]].all(), d
        nearest = np.where(shrunk[pix], rho[None, :], np.inf).min(-1)
        chosen = rho[g[pix]]
        assert (nearest >= chosen * (1 - 1e-5)).all(), d


@pytest.mark.parametrize("scene,max_splat", CASES, ids=IDS)
def test_index_is_exact_where_the_reference_is_decided(scene, max_splat):
    res = wr.reference(scene, max_splat)
    got = run(scene, max_splat)["index"].reshape(3, -1)
    firm = ~wr.fragile(res)
    share = firm.mean()
    print(scene["name"], max_splat, "non-fragile share", share, "mismatches", (got != res["index"].reshape(3, -1))[firm].sum())
    assert share >= 0.9
    assert np.array_equal(got[firm], res["index"].reshape(3, -1)[firm])


@pytest.mark.parametrize("scene,max_splat", CASES, ids=IDS)
def test_resolve_outputs(scene, max_splat):
    """image: the source gathered by the kernel's own index, bit for bit (from a permuted [S, H, W, C] view as well);
    depth |d_dst|: the fp32 rho of that point as the reference's fp32 mode states it on the device's own ray directions
    (every later operation is a correctly rounded +, -, *, / or sqrt in a stated order), within 4 ulp; holes: fill, NaN, 0"""
    from pano_nerf_amd import views
    src, dst = scene["src"], scene["dst"]
    out = run(scene, max_splat)
    img = _image(scene)
    idx = out["index"]
    hit = idx >= 0
    assert 0.05 < hit.mean() < 1.0 or max_splat > 1
    flat = np.moveaxis(img, 1, 0).reshape(3, -1)
    want = np.where(hit[:, None], np.moveaxis(flat[:, np.where(hit, idx, 0)], 0, 1), np.float32(FILL))
    assert out["image"].shape == want.shape and np.array_equal(bits(out["image"]), bits(want))
    assert np.array_equal(out["coverage"], hit.astype(np.float32))
    assert out["depth"].shape == (3, 1, dst.h, dst.w) and np.isnan(out["depth"][:, 0][~hit]).all()
    # the same image held as [S, H, W, C] and passed as a permuted view
    nhwc = torch.from_numpy(np.ascontiguousarray(np.moveaxis(img, 1, -1))).to(dev())
    again = views.warp_view(nhwc.permute(0, 3, 1, 2), torch.from_numpy(scene["depth"]).to(dev())[:, None], src,
                            scene["src_c2ws"], dst, scene["dst_c2ws"], max_splat=max_splat, fill=FILL)
    assert np.array_equal(bits(again["image"].cpu().numpy()), bits(out["image"]))
    assert np.array_equal(again["index"].cpu().numpy(), idx)
    # depth
    dirs = [views.generate_camera_rays(src, c, device=dev()).directions.cpu().numpy() for c in scene["src_c2ws"]]
    f32 = wr.warp(src, scene["src_c2ws"], scene["depth"], dst, scene["dst_c2ws"], max_splat, dt=np.float32, world_dirs=dirs)
    nd = np.ones((dst.h, dst.w), np.float32)
    if cr.kind(dst) == "pinhole":
        jj, ii = np.meshgrid(np.arange(dst.w, dtype=np.float32), np.arange(dst.h, dtype=np.float32))
        nd = wr._norm(cr.pix_to_dir(dst, jj + np.float32(0.5), ii + np.float32(0.5), np.float32)[0])
        assert nd.dtype == np.float32
    worst = 0.0
    for d in range(3):
        rho = f32["rho"][d][idx[d][hit[d]]]
        assert rho.dtype == np.float32
        got = out["depth"][d, 0][hit[d]] * nd[hit[d]]
        ulps = np.abs(got.astype(np.float64) - rho) / np.spacing(rho).astype(np.float64)
        worst = max(worst, float(ulps.max()) if ulps.size else 0.0)
    print(scene["name"], max_splat, "depth |d_dst| against the fp32 rho: worst", worst, "ulp")
    assert worst <= 4.0


def test_repeatable_and_index_only():
    from pano_nerf_amd import views
    scene = wr.SCENES[0]
    first = run(scene, 4)
    img = torch.from_numpy(_image(scene)).to(dev())
    dep = torch.from_numpy(scene["depth"]).to(dev())
    again = views.warp_view(img, dep, scene["src"], scene["src_c2ws"], scene["dst"], scene["dst_c2ws"], max_splat=4, fill=FILL)
    assert sorted(again) == ["coverage", "depth", "image", "index"]
    for k in again:
        a, b = again[k].cpu().numpy(), first[k]
        assert np.array_equal(a, b) if a.dtype == np.int64 else np.array_equal(bits(a), bits(b)), k
    bare = views.warp_view(None, dep, scene["src"], scene["src_c2ws"], scene["dst"], scene["dst_c2ws"], max_splat=4)
    assert sorted(bare) == ["coverage", "depth", "index"]
    assert np.array_equal(bare["index"].cpu().numpy(), first["index"])
    assert np.array_equal(bits(bare["depth"].cpu().numpy()), bits(first["depth"]))
    # one frame, one pose, no batch dimensions
    one = views.warp_view(img[0], dep[0], scene["src"], scene["src_c2ws"][0], scene["dst"], scene["dst_c2ws"][1][:3], max_splat=4)
    assert one["image"].shape == (1, 3, scene["dst"].h, scene["dst"].w) and one["index"].shape == (1, scene["dst"].h, scene["dst"].w)
    assert int(one["index"].max()) < scene["src"].h * scene["src"].w


def test_error_paths():
    from pano_nerf_amd import views, _lib
    from pano_nerf_amd.cameras import _kind_params
    pano, pin = views.pano_camera(8, 16), views.perspective_camera(6, 8, fov_x_deg=60.0)
    stereo = views.stereo_pano_camera(8, 16, 0.06, "left")
    img = torch.zeros(1, 3, 8, 16, device=dev())
    dep = torch.ones(1, 8, 16, device=dev())
    eye = np.eye(4)
    ok = dict(image=img, depth=dep, src_camera=pano, src_c2w=eye, dst_camera=pin, dst_c2w=eye)
    views.warp_view(**ok)
    for change, exc in ((dict(src_camera=stereo), ValueError), (dict(dst_camera=stereo), ValueError),
                        (dict(depth=torch.ones(1, 8, 15, device=dev())), ValueError),
                        (dict(image=torch.zeros(1, 3, 7, 16, device=dev())), ValueError),
                        (dict(image=torch.zeros(2, 3, 8, 16, device=dev())), ValueError),
                        (dict(src_c2w=np.stack([eye, eye])), ValueError), (dict(dst_c2w=np.eye(3)), ValueError),
                        (dict(max_splat=0), ValueError), (dict(max_splat=9), ValueError), (dict(max_splat=2.5), ValueError),
                        (dict(splat_scale=0.0), ValueError), (dict(splat_scale=float("nan")), ValueError),
                        (dict(depth=dep.cpu()), RuntimeError), (dict(image=img.cpu()), RuntimeError)):
        with pytest.raises(exc):
            views.warp_view(**{**ok, **change})
    # the C entry points return the stated codes for the same inputs (no launch: zbuf keeps its bits)
    lib = _lib.load()
    (pk, pp), (hk, hp) = _kind_params(pano), _kind_params(pin)
    m = torch.eye(4, device=dev()).reshape(1, 16).contiguous()
    zbuf = torch.full((1, 6, 8), -1, dtype=torch.int64, device=dev())

    def splat(sk=pk, hs=8, ws=16, dk=hk, hd=6, wd=8, max_splat=4, scale=1.0, S=1, D=1):
        return lib.pn_warp_splat(S, sk, hs, ws, pp.ctypes.data, dep.data_ptr(), m.data_ptr(), D, dk, hd, wd, hp.ctypes.data,
                                 m.data_ptr(), max_splat, scale, zbuf.data_ptr(), None)

    BAD_SHAPE, UNSUPPORTED = -1, -2
    assert splat(sk=4) == UNSUPPORTED and splat(dk=4) == UNSUPPORTED and splat(sk=7) == UNSUPPORTED
    assert splat(max_splat=0) == BAD_SHAPE and splat(max_splat=9) == BAD_SHAPE
    assert splat(scale=0.0) == BAD_SHAPE and splat(scale=-1.0) == BAD_SHAPE
    assert splat(hs=1) == BAD_SHAPE and splat(wd=1) == BAD_SHAPE and splat(sk=2) == BAD_SHAPE  # a cube needs H = 6 W
    assert splat(S=1 << 25) == BAD_SHAPE  # S Hs Ws = 2^32
    assert splat(D=1 << 26, hd=4, wd=8) == BAD_SHAPE  # D Hd Wd = 2^31
    idx = torch.empty(1, 6, 8, dtype=torch.int64, device=dev())
    f = torch.empty(1, 6, 8, device=dev())
    assert lib.pn_warp_resolve(1, 0, 8, 16, 1, 4, 6, 8, hp.ctypes.data, zbuf.data_ptr(), None, 0, 0, 0, 0.0, None,
                               f.data_ptr(), idx.data_ptr(), f.data_ptr(), None) == UNSUPPORTED
    assert lib.pn_warp_resolve(1, 0, 8, 16, 1 << 26, hk, 4, 8, hp.ctypes.data, zbuf.data_ptr(), None, 0, 0, 0, 0.0, None,
                               f.data_ptr(), idx.data_ptr(), f.data_ptr(), None) == BAD_SHAPE
    torch.cuda.synchronize()
    assert bool((zbuf == -1).all())
    assert lib.pn_abi_version() == 2


# ------------------------------------------------------------------------------------------------ render_path_warped
def make_model():
    """the tiny model of tests/test_gpu_views.py"""
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


def test_render_path_warped():
    from pano_nerf_amd import views
    model = make_model()
    H, W, n = 12, 16, 5
    cam = views.perspective_camera(H, W, fov_x_deg=60.0)
    poses = np.stack([views.look_at([0.15 * i - 0.3, 0.05 * i, 2.0 - 0.1 * i], [0, 0, 0]) for i in range(n)])
    kinds = ("ldr", "depth", "hdr")
    full = views.render_path(model, cam, poses, kinds=kinds, near=0.0, far=10.0, exposure=0.5)
    every = views.render_path_warped(model, cam, poses, 1, kinds=kinds, near=0.0, far=10.0, exposure=0.5)
    assert sorted(every) == sorted(kinds + ("coverage",))
    for k in kinds:
        assert same(every[k], full[k]), k
    assert every["coverage"].shape == (n, H, W) and bool((every["coverage"] == 1).all())
    got = views.render_path_warped(model, cam, poses, 2, kinds=kinds, near=0.0, far=10.0, exposure=0.5, max_splat=3)
    for i in (0, 2, 4):
        for k in kinds:
            assert same(got[k][i], full[k][i]), (k, i)
        assert bool((got["coverage"][i] == 1).all())
    for i in (1, 3):
        v = [views.render_view(model, cam, poses[j], outputs=("rgb", "depth")) for j in (i - 1, i + 1)]
        w = views.warp_view(torch.cat([v[0]["fine_rgb"], v[1]["fine_rgb"]]), torch.cat([v[0]["fine_dep"], v[1]["fine_dep"]]),
                            cam, poses[[i - 1, i + 1]], cam, poses[i], max_splat=3)
        assert 0.1 < float(w["coverage"].mean())
        assert same(got["hdr"][i], w["image"][0].permute(1, 2, 0)), i
        assert same(got["ldr"][i], views.to_frame(w["image"], "ldr", exposure=0.5)), i
        assert same(got["depth"][i], views.to_frame(w["depth"], "depth", 0.0, 10.0)), i
        assert same(got["coverage"][i], w["coverage"][0]), i
    # three poses at key_every = 5: the last pose is rendered too
    last = views.render_path_warped(model, cam, poses[:3], 5, kinds=("hdr",))
    assert same(last["hdr"][2], full["hdr"][2]) and bool((last["coverage"][[0, 2]] == 1).all())
    for bad in ("normal", "albedo", "ldr_surf"):
        with pytest.raises(ValueError, match=bad):
            views.render_path_warped(model, cam, poses, 2, kinds=("ldr", bad))
    with pytest.raises(ValueError):
        views.render_path_warped(model, cam, poses, 0)
