"""Cube-map, fisheye and stereo-panorama cameras and views.reproject on the GPU: rays and reprojection against the fp64
restatement of tests/_cameras_ref.py, the consumers (render_view, render_stereo_pano, render_path, insert_object,
probes_to_cubemaps) against the composition of their public pieces bit for bit, and the entry points' error codes."""
import ctypes
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import _cameras_ref as ref

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)  # 2^-23
# Source-coordinate uncertainty of one subsample, in units of EPS x scale (scale = Ws / (2 pi sin phi) for a panorama's
# column, max(Hs, Ws) for every other coordinate): MEASURED reference against reference - the fp32 run of the numpy
# restatement against its fp64 run, over every (src, dst, samples) case of test_reproject_matches_the_fp64_restatement -
# as 4.273 at most (ref.coord_error; test_coordinate_constant_is_the_measured_one keeps the figure honest).  x 4 margin.
C_MEASURED = 4.3
C_COORD = 4 * C_MEASURED
ROT = ref.rotation_matrix((0.3, -0.8, 0.52), 1.234)


def dev():
    return torch.device("cuda:0")


def T(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).to(dev())


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


_MODELS = {}


def model():
    if "m" not in _MODELS:
        import pano_nerf_amd as pn
        from oracle import pano_oracle as orc
        m = pn.PanoMipNeRF(num_samples=16, rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
        m.mlp.load_state_dict(orc.init_params(4, 5))
        m = m.to(dev())
        m.mlp_mode = "fused_f16x2"
        _MODELS["m"] = m
    return _MODELS["m"]


def generic_c2w(k=0):
    c = np.eye(4)
    c[:3, :3] = ref.rotation_matrix((0.2 + k, 0.9, -0.4), 0.7 + 0.9 * k)
    c[:3, 3] = (0.3 - k, -0.2, 0.5 + 0.25 * k)
    return c.astype(np.float32)


# --------------------------------------------------------------------------------------------------------------- rays
def ray_cameras():
    from pano_nerf_amd import views
    return dict(cube2=views.cubemap_camera(2), cube3=views.cubemap_camera(3),
                fisheye180=views.fisheye_camera(5, 7, fov_deg=180.0), fisheye360=views.fisheye_camera(4, 4, fov_deg=360.0),
                stereo_left=views.stereo_pano_camera(4, 8, 0.064, "left"),
                stereo_right=views.stereo_pano_camera(4, 8, 0.064, "right"))


def _take(cam, c2ws, idx, rgb_pool, near=0.25, far=7.5):
    from pano_nerf_amd import views
    return views.CameraRig(cam, views._c2w_stack(c2ws), dev()).sample(idx, near, far, rgb_pool)


def _shuffled_rows(cam, n_cam, seed):
    """every (camera, pixel) row once, shuffled, then one row outside the pool (it reads ray 0)"""
    rows = np.random.default_rng(seed).permutation(n_cam * cam.h * cam.w)
    return np.concatenate([rows, [n_cam * cam.h * cam.w + 5]])


@pytest.mark.parametrize("name", list(ray_cameras()))
def test_rays_match_the_fp64_restatement(name):
    """Absolute 2e-6 per unit-vector component (a few ulp of sin / cos / atan2 at arguments up to 2 pi, ulp 4.8e-7, plus a
    3-term rotation); origins 2e-6 (|t| + ipd); radii 4e-6 of the direction scale (1); the rest exact."""
    cam = ray_cameras()[name]
    c2ws = [generic_c2w(0), generic_c2w(1)]
    hw = cam.h * cam.w
    rows = _shuffled_rows(cam, 2, 7)
    pool = np.random.default_rng(8).random((2 * hw, 3)).astype(np.float32)
    got, rgb = _take(cam, c2ws, T(rows, torch.int64), T(pool))
    want = [ref.rays(cam, c, 0.25, 7.5) for c in c2ws]
    src = np.where(rows < 2 * hw, rows, 0)
    want = {f: np.concatenate([w[f] for w in want], 0)[src] for f in want[0]}
    g = {f: getattr(got, f).cpu().numpy().astype(np.float64) for f in got._fields}
    ipd = getattr(cam, "ipd", 0.0)
    tnorm = max(float(np.linalg.norm(c[:3, 3])) for c in c2ws)
    err = {f: float(np.abs(g[f] - want[f]).max()) for f in g}
    print(name, {k: f"{v:.2e}" for k, v in err.items()})
    assert err["directions"] <= 2e-6 and err["viewdirs"] <= 2e-6
    assert err["origins"] <= 2e-6 * (tnorm + ipd)
    assert err["radii"] <= 4e-6
    assert err["lossmult"] == 0 and err["near"] == 0 and err["far"] == 0
    if name.startswith("stereo"):
        assert err["noise_var"] <= 2e-6 * math_pi_over(cam.w)
        t = np.stack([c[:3, 3] for c in c2ws])[src // hw].astype(np.float64)
        assert np.abs(np.linalg.norm(g["origins"] - t, axis=-1) - ipd / 2).max() <= 2e-6 * (tnorm + ipd)
    else:
        assert err["noise_var"] == 0 and not g["noise_var"].any()
        assert np.array_equal(g["directions"], g["viewdirs"])
    if name.startswith("fisheye"):
        assert 0 < (g["lossmult"] == 0).sum() < len(rows)  # both sides of the image circle are covered
    assert np.array_equal(rgb.cpu().numpy(), pool[src])
    # without target colours
    again, none = _take(cam, c2ws, T(rows, torch.int64), None)
    assert none is None and all(bits_equal(getattr(again, f), getattr(got, f)) for f in got._fields)


def math_pi_over(w):
    return float(np.pi) / w


@pytest.mark.parametrize("eye", ["left", "right"])
def test_stereo_pano_with_zero_ipd_is_the_pano_camera_bit_for_bit(eye):
    from pano_nerf_amd import views
    H, W = 4, 8
    c2ws = [generic_c2w(0), generic_c2w(1)]
    rows = T(_shuffled_rows(views.pano_camera(H, W), 2, 9), torch.int64)
    pool = T(np.random.default_rng(10).random((2 * H * W, 3)).astype(np.float32))
    a, argb = _take(views.stereo_pano_camera(H, W, 0.0, eye), c2ws, rows, pool)
    b, brgb = _take(views.pano_camera(H, W), c2ws, rows, pool)
    for f in a._fields:
        assert bits_equal(getattr(a, f), getattr(b, f)), f
    assert bits_equal(argb, brgb)


def test_generate_camera_rays_is_every_camera():
    import pano_nerf_amd as pn
    from pano_nerf_amd import views
    c2w = generic_c2w(0)
    pin = views.perspective_camera(6, 8, fov_x_deg=70.0)
    for a, b in ((views.generate_camera_rays(pin, c2w), views.generate_perspective_rays(pin, c2w)),
                 (views.generate_camera_rays(views.pano_camera(4, 8), c2w), pn.generate_pano_rays(4, 8, c2w))):
        assert all(bits_equal(getattr(a, f), getattr(b, f)) for f in a._fields)
    cube = views.generate_camera_rays(views.cubemap_camera(3), c2w, 0.5, 4.0)
    assert cube.origins.shape == (54, 3) and cube.radii.shape == (54, 1)
    want = ref.rays(views.cubemap_camera(3), c2w, 0.5, 4.0)
    assert np.abs(cube.directions.cpu().numpy() - want["directions"]).max() <= 2e-6
    with pytest.raises(RuntimeError):
        views.generate_camera_rays(views.cubemap_camera(3), c2w, device="cpu")


def pool_cameras():
    from pano_nerf_amd import views
    cams = dict(pano=views.pano_camera(4, 8), pinhole=views.perspective_camera(6, 8, fov_x_deg=70.0), **ray_cameras())
    for eye in ("left", "right"):
        cams[f"stereo_{eye}_ipd0"] = views.stereo_pano_camera(4, 8, 0.0, eye)
    return cams


@pytest.mark.parametrize("name", list(pool_cameras()))
def test_ray_pool_take_is_generate_camera_rays_row_for_row(name):
    """The decode and store path every camera shares: RayPool.take of every row once, shuffled, plus a row below 0 and a
    row >= len(pool), equals the per-camera generate_camera_rays rows bit for bit; both outside rows read row 0, colour
    included.  B = 2 H W + 2 is no multiple of the block size, so the last workgroup is partial."""
    from pano_nerf_amd import views
    from pano_nerf_amd.rays import CameraRig, RayPool
    cam = pool_cameras()[name]
    c2ws = [generic_c2w(0), generic_c2w(1)]
    n = 2 * cam.h * cam.w
    images = np.random.default_rng(12).random((2, cam.h, cam.w, 3)).astype(np.float32)
    pool = RayPool(CameraRig(cam, np.stack(c2ws), dev()), images, near=0.25, far=7.5)
    assert len(pool) == n
    rows = np.concatenate([np.random.default_rng(11).permutation(n), [-3, n + 5]])
    got, rgb = pool.take(T(rows, torch.int64))
    full = [views.generate_camera_rays(cam, c, 0.25, 7.5) for c in c2ws]
    src = torch.as_tensor(np.where((rows >= 0) & (rows < n), rows, 0)).to(dev())
    assert len(rows) == n + 2 and (src[-2:] == 0).all()
    for f in got._fields:
        assert bits_equal(getattr(got, f), torch.cat([getattr(r, f) for r in full], 0)[src]), f
    assert bits_equal(rgb, T(images.reshape(n, 3))[src])


# ------------------------------------------------------------------------------------------------------- reprojection
def central_cameras():
    from pano_nerf_amd import views
    return dict(pano=views.pano_camera(8, 16), pinhole=views.perspective_camera(6, 8, fov_x_deg=90.0),
                cube=views.cubemap_camera(4), fisheye=views.fisheye_camera(9, 9, fov_deg=220.0))


def smooth_image(cam, N, C):
    """[N, C, H, W] fp32: a smooth function of the pixel's direction (a fisheye's formula continues outside its circle),
    and (Gh, Gv), its largest horizontal / vertical adjacent-pixel differences (a panorama's columns wrap; a cube's
    neighbours are within a face, as its taps are)"""
    px, py = np.meshgrid(np.arange(cam.w) + 0.5, np.arange(cam.h) + 0.5)
    d, _ = ref.pix_to_dir(cam, px, py)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    img = np.empty((N, C, cam.h, cam.w))
    for n in range(N):
        for c in range(C):
            a = np.array([0.6 - 0.5 * c, 0.3 + 0.2 * n, 0.5 * c - 0.4])
            b = np.array([0.2, -0.7 + 0.3 * c, 0.6 - 0.4 * n])
            img[n, c] = 1.5 + 0.25 * n + 0.6 * (d @ a) + 0.5 * (d @ b) ** 2
    img = img.astype(np.float32)
    i64 = img.astype(np.float64)
    gh = np.abs(np.diff(i64, axis=-1)).max()
    if ref.kind(cam) == "pano":
        gh = max(gh, np.abs(i64[..., 0] - i64[..., -1]).max())
    if ref.kind(cam) == "cube":
        gv = np.abs(np.diff(i64.reshape(N, C, 6, cam.w, cam.w), axis=-2)).max()
    else:
        gv = np.abs(np.diff(i64, axis=-2)).max()
    return img, float(gh), float(gv)


def sample_tolerance(src, info, gh, gv, vmax):
    """per subsample: Gh dx + Gv dy + 4 EPS max|image|, dx = C EPS Ws / (2 pi sin phi) for a panorama source (longitude is
    ill-conditioned near a pole and the bound says so) and C EPS max(Hs, Ws) otherwise, dy = C EPS max(Hs, Ws)"""
    big = float(max(src.h, src.w))
    dy = C_COORD * EPS * big
    dx = C_COORD * EPS * src.w / (2 * np.pi * np.maximum(info["sin_phi"], 1e-300)) if ref.kind(src) == "pano" else dy
    return gh * dx + gv * dy + 4 * EPS * vmax


def decided(src, info):
    """subsamples far enough from every discrete decision fp32 may flip: a cube face tie (two largest |components|
    within 1e-5 relative), a pinhole frustum border or a fisheye image circle (within 1e-4 px)"""
    return info["margin"] >= (1e-5 if ref.kind(src) == "cube" else 1e-4)


PAIRS = [(s, d) for s in ("pano", "pinhole", "cube", "fisheye") for d in ("pano", "pinhole", "cube", "fisheye")]


def test_coordinate_constant_is_the_measured_one():
    """reference against reference (no kernel): the fp32 restatement's source coordinates stay within C_MEASURED of the
    fp64 one's in every case below (x 1.5: numpy's fp32 sin / cos / arctan2 differ by an ulp between builds)"""
    cams = central_cameras()
    worst = 0.0
    for s, d in PAIRS:
        for k in (1, 3):
            rx, ry = ref.coord_error(cams[s], cams[d], ROT, k)
            worst = max([worst] + list(rx) + list(ry))
    print("fp32 restatement against fp64: worst coordinate error", worst, "EPS scale")
    assert worst <= 1.5 * C_MEASURED


@pytest.mark.parametrize("src_name,dst_name", PAIRS)
def test_reproject_matches_the_fp64_restatement(src_name, dst_name):
    from pano_nerf_amd import views
    cams = central_cameras()
    src, dst = cams[src_name], cams[dst_name]
    N = 2
    for C in (1, 3):
        img, gh, gv = smooth_image(src, N, C)
        vmax = float(np.abs(img).max())
        if C == 3:  # a [N, C, H, W] view of an [N, H, W, C] buffer, read in place
            x = T(img.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2)
            assert not x.is_contiguous()
        else:
            x = T(img)
        for k in (1, 3):
            info = ref.sample_coords(src, dst, ROT, k)
            want, wcov = ref.reproject(img, src, dst, ROT, k, fill=-2.5, info=info)
            got, cov = views.reproject(x, src, dst, rotation=ROT, samples=k, fill=-2.5)
            assert got.shape == (N, C, dst.h, dst.w) and cov.shape == (dst.h, dst.w) and got.is_contiguous()
            again, cov2 = views.reproject(x, src, dst, rotation=ROT, samples=k, fill=-2.5)
            assert bits_equal(got, again) and bits_equal(cov, cov2)  # no atomics: the same bits
            got, cov = got.cpu().numpy().astype(np.float64), cov.cpu().numpy().astype(np.float64)
            ok = decided(src, info)
            tol = sample_tolerance(src, info, gh, gv, vmax)
            loose = ~ok | (info["valid"] & (tol > 1e-4 * vmax))
            print(f"{src_name}->{dst_name} C={C} k={k}: {int((~ok).sum())} undecided + {int((loose & ok).sum())} loose of "
                  f"{ok.size} subsamples; min sin phi {float(info['sin_phi'].min()):.3f}")
            assert loose.sum() <= 0.01 * ok.size
            pix_ok = ok.all(-1)
            nvalid = info["valid"].sum(-1)
            pix_tol = np.where(nvalid > 0, np.where(info["valid"], tol, 0.0).sum(-1) / np.maximum(nvalid, 1), 0.0)
            err = np.abs(got - want)
            worst = float((err / np.maximum(pix_tol, 1e-300))[:, :, pix_ok & (nvalid > 0)].max()) if (pix_ok & (nvalid > 0)).any() else 0.0
            print(f"    worst error / tolerance {worst:.3f}; max error {float(err[:, :, pix_ok].max()) if pix_ok.any() else 0.0:.2e}")
            assert (err[:, :, pix_ok] <= pix_tol[pix_ok]).all()
            assert np.array_equal(cov[pix_ok], wcov[pix_ok].astype(np.float32).astype(np.float64))
            empty = pix_ok & (nvalid == 0)
            assert (got[:, :, empty] == -2.5).all()
            if src_name in ("pinhole", "fisheye") and dst_name in ("pano", "cube"):
                assert empty.any()  # a source that does not see the whole sphere: the case does cover `fill`
    # the default rotation is the identity
    a, _ = views.reproject(x, src, dst)
    b, _ = views.reproject(x, src, dst, rotation=np.eye(3))
    assert bits_equal(a, b)


@pytest.mark.parametrize("src_name,dst_name", [("pano", "cube"), ("cube", "fisheye"), ("fisheye", "pano")])
def test_reproject_propagates_nan(src_name, dst_name):
    """a NaN source pixel makes every output it touches NaN and no other: `touches` is decided by the fp64 restatement
    with margins - outputs whose taps give the NaN pixel a weight above 1e-3 must be NaN; outputs that stay finite even
    when the NaN pixel's eight neighbours are NaN too must be finite"""
    from pano_nerf_amd import views
    cams = central_cameras()
    src, dst = cams[src_name], cams[dst_name]
    img, _, _ = smooth_image(src, 1, 1)
    y, x = (2, 5) if src_name == "pano" else ((5, 1) if src_name == "cube" else (4, 5))  # interior of the image / a face
    bad = img.copy()
    bad[0, 0, y, x] = np.nan
    wide = img.copy()
    wide[0, 0, y - 1:y + 2, x - 1:x + 2] = np.nan
    info = ref.sample_coords(src, dst, ROT, 2)
    one = np.zeros_like(img)
    one[0, 0, y, x] = 1.0
    weight, _ = ref.reproject(one, src, dst, ROT, 2, info=info)
    wide_out, _ = ref.reproject(wide, src, dst, ROT, 2, info=info)
    got, _ = views.reproject(T(bad), src, dst, rotation=ROT, samples=2)
    got = got.cpu().numpy()
    pix_ok = decided(src, info).all(-1)
    must = pix_ok & (weight[0, 0] > 1e-3)
    must_not = pix_ok & np.isfinite(wide_out[0, 0])
    assert must.any() and must_not.any()
    assert np.isnan(got[0, 0][must]).all() and np.isfinite(got[0, 0][must_not]).all()


def test_probes_to_cubemaps_is_reproject():
    from pano_nerf_amd import lighting, views
    g = torch.Generator().manual_seed(3)
    probes = (torch.rand(3, 8, 16, 3, generator=g) * 4.0).to(dev()).permute(0, 3, 1, 2)  # as light_probes returns them
    cubes = lighting.probes_to_cubemaps(probes, 5)
    assert cubes.shape == (3, 3, 30, 5)
    want, cov = views.reproject(probes, views.pano_camera(8, 16), views.cubemap_camera(5), samples=4)
    assert bits_equal(cubes, want) and bool((cov == 1).all())
    assert bits_equal(lighting.probes_to_cubemaps(probes, 5, samples=1),
                      views.reproject(probes.contiguous(), views.pano_camera(8, 16), views.cubemap_camera(5))[0])
    assert views.cube_faces(cubes).shape == (3, 6, 3, 5, 5)
    with pytest.raises(RuntimeError):
        lighting.probes_to_cubemaps(probes.cpu(), 5)


# ------------------------------------------------------------------------------------------------------- composition
def _by_hand(rays, H, W, env):
    import pano_nerf_amd as pn
    names = ("coarse_rgb", "fine_rgb", "coarse_dep", "fine_dep", "fine_nor", "albedo", "roughness", "surface_rgb", "shading")
    return dict(zip(names, pn.render_image(model(), pn.Rays(*[x.view(1, H, W, -1) for x in rays]), env, H, W)))


def test_render_view_of_a_cube_map_is_the_renderer():
    import pano_nerf_amd as pn
    from pano_nerf_amd import views
    cam = views.cubemap_camera(3)
    c2w = generic_c2w(0)
    env = pn.generate_lit_rays(10, 0.01)
    img = _by_hand(views.generate_camera_rays(cam, c2w), cam.h, cam.w, env)
    out = views.render_view(model(), cam, c2w, env, outputs=("rgb", "depth", "normal", "shading"), chunk_rays=17)
    for k, v in out.items():
        assert v.shape == (1, v.shape[1], 18, 3) and bits_equal(v, img[k]), k


def test_render_stereo_pano_is_two_render_views():
    from pano_nerf_amd import views
    H, W, ipd = 4, 8, 0.064
    c2w = generic_c2w(1)
    out = views.render_stereo_pano(model(), H, W, ipd, c2w, outputs=("rgb", "depth"))
    left, right = (views.render_view(model(), views.stereo_pano_camera(H, W, ipd, eye), c2w, outputs=("rgb", "depth"))
                   for eye in ("left", "right"))
    assert sorted(out) == sorted(left)
    for k in out:
        assert out[k].shape == (1, left[k].shape[1], 2 * H, W)
        assert bits_equal(out[k], torch.cat([left[k], right[k]], 2)), k
    assert not bits_equal(left["fine_rgb"], right["fine_rgb"])  # the eyes do differ


def test_fisheye_render_view_is_zero_outside_the_circle():
    import pano_nerf_amd as pn
    from pano_nerf_amd import views
    cam = views.fisheye_camera(6, 8, fov_deg=200.0)
    c2w = generic_c2w(0)
    mask = torch.from_numpy(views.camera_mask(cam)).to(dev())
    assert 0 < int(mask.sum()) < mask.numel()
    rays = views.generate_camera_rays(cam, c2w)
    assert bits_equal(rays.lossmult.view(6, 8), mask.float())
    img = _by_hand(rays, cam.h, cam.w, pn.generate_lit_rays(10, 0.01))
    out = views.render_view(model(), cam, c2w, outputs=("rgb", "depth", "normal"))
    for k, v in out.items():
        assert bool((v[0][:, ~mask] == 0).all()), k
        assert bits_equal(v[0][:, mask], img[k][0][:, mask]), k
        assert bool((v[0][:, mask] != 0).any()), k


def _read_png(path):
    """decode write_png's output (8-bit RGB, filter type 0 on every row) with zlib"""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        (length,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + length]
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + length
    w, h, depth, ctype = hdr[:4]
    assert depth == 8 and ctype == 2
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 3)


def test_render_path_writes_cube_strips(tmp_path):
    from pano_nerf_amd import io_exr, views
    S, n = 4, 2
    cam = views.cubemap_camera(S)
    poses = np.stack([generic_c2w(0), generic_c2w(1)]).astype(np.float64)
    kinds = ("ldr", "depth", "hdr")
    fr = views.render_path(model(), cam, poses, kinds=kinds, chunk_rays=50)
    assert fr["ldr"].shape == (n, 6 * S, S, 3)
    for i in range(n):
        v = views.render_view(model(), cam, poses[i], outputs=("rgb", "depth"))
        assert bits_equal(fr["ldr"][i], views.to_frame(v["fine_rgb"], "ldr"))
    assert views.render_path(model(), cam, poses, kinds=kinds, chunk_rays=50, out_dir=str(tmp_path)) == {}
    for k in kinds:
        ext = "exr" if k == "hdr" else "png"
        assert sorted(os.listdir(tmp_path / k)) == [f"{i:05d}.{ext}" for i in range(n)]
        for i in range(n):
            path = str(tmp_path / k / f"{i:05d}.{ext}")
            back = io_exr.read_exr(path) if k == "hdr" else _read_png(path)
            assert back.shape == (6 * S, S, 3) and np.array_equal(back, fr[k][i].cpu().numpy()), (k, i)


def test_insert_object_with_a_fisheye_camera():
    """insert_object takes the new cameras through the rays render_view renders: the hand composition of the public
    pieces, bit for bit.  The sphere sits off the axis, so the forward rays of the pixels outside the circle miss it."""
    from pano_nerf_amd import lighting, objects, views
    _spec = importlib.util.spec_from_file_location("_objects_spec", os.path.join(os.path.dirname(__file__), "test_objects_cpu.py"))
    spec = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(spec)
    cam = views.fisheye_camera(20, 24, fov_deg=180.0)
    H, W = cam.h, cam.w
    c2w = np.eye(4)
    v, f = spec.icosphere(1, 0.2, (0.25, 0.1, -0.6))
    obj = objects.VirtualObject(T(v), T(f, torch.int32))
    out = objects.insert_object(model(), cam, c2w, obj, probe_size=(8, 16), shadows=False)
    inside = torch.from_numpy(views.camera_mask(cam)).to(dev())
    m = out["mask"][0, 0] > 0
    print("fisheye insert: masked pixels", int(m.sum()), "of", m.numel(), "inside the circle", int((m & inside).sum()))
    assert int((m & inside).sum()) > 0 and int((m & ~inside).sum()) == 0
    assert all(bool(torch.isfinite(x).all()) for x in out.values())
    # by hand
    scene = views.render_view(model(), cam, c2w, outputs=("rgb", "depth", "normal"))
    rows = lambda x: x.permute(0, 2, 3, 1).reshape(H * W, -1)
    rays = views.generate_camera_rays(cam, c2w)
    t, face, bary = objects.trace_mesh(rays.origins, rays.directions, obj.vertices, obj.faces)
    at = objects.hit_attributes(obj, rays.origins, rays.directions, t, face, bary, rows(scene["fine_dep"]), None)
    mk = at["mask"]
    probes = lighting.light_probes(model(), obj.centroid(), 8, 16)
    object_rgb = torch.zeros(H * W, 3, device=dev())
    object_rgb[mk] = objects.shade(probes, at["albedo"][mk], at["normals"][mk], at["viewdirs"][mk], obj.roughness, None)[0]
    rgb = torch.where(mk[:, None], object_rgb, rows(scene["fine_rgb"]))
    depth = torch.where(mk, t, rows(scene["fine_dep"])[:, 0])
    img = lambda x: x.reshape(1, H, W, -1).permute(0, 3, 1, 2)
    assert bits_equal(out["mask"], img(mk.float())) and bits_equal(out["object_rgb"], img(object_rgb))
    assert bits_equal(out["rgb"], img(rgb)) and bits_equal(out["depth"], img(depth))
    assert bool((out["scene_rgb"][0][:, ~inside] == 0).all())


# ------------------------------------------------------------------------------------------------------------- errors
def test_entry_point_errors():
    from pano_nerf_amd import _lib
    lib = _lib.load()
    BAD_SHAPE, UNSUPPORTED = -1, -2
    buf = torch.zeros(64, dtype=torch.float32, device=dev())
    idx = torch.zeros(4, dtype=torch.int64, device=dev())
    params = (ctypes.c_float * 20)(*([1.0, 1.0] + [0.0] * 18))
    eye = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    p = buf.data_ptr()
    CUBE, FISHEYE, STEREO, PANO, PINHOLE = 2, 3, 4, 0, 1

    def sample(kind, H, W, B=4, n_cam=1):
        return lib.pn_sample_camera_rays(B, n_cam, kind, H, W, params, idx.data_ptr(), p, 0.0, 1.0, None, p, p, p, p, p, p,
                                         p, p, None, None)

    assert sample(CUBE, 6, 1) == BAD_SHAPE and sample(CUBE, 13, 2) == BAD_SHAPE  # size < 2; not a 6 S x S strip
    assert sample(FISHEYE, 1, 8) == BAD_SHAPE and sample(FISHEYE, 8, 1) == BAD_SHAPE
    assert sample(STEREO, 4, 2) == BAD_SHAPE and sample(STEREO, 1, 8) == BAD_SHAPE
    assert sample(FISHEYE, 65536, 32768) == BAD_SHAPE and sample(CUBE, 6 * 18919, 18919) == BAD_SHAPE  # H W >= 2^31
    assert sample(CUBE, 12, 2, B=0) == BAD_SHAPE and sample(CUBE, 12, 2, n_cam=0) == BAD_SHAPE
    for kind in (PANO, PINHOLE, 5, -1, 99):  # the panorama and the pinhole keep their own entry points
        assert sample(kind, 12, 2) == UNSUPPORTED

    def reproject(sk, Hs, Ws, dk, Hd, Wd, samples=1, N=1, C=1):
        return lib.pn_reproject(N, C, sk, Hs, Ws, params, dk, Hd, Wd, params, eye, samples, 0.0, p, 0, 0, 1, p, p, None)

    assert reproject(PANO, 4, 8, CUBE, 12, 2, samples=0) == BAD_SHAPE and reproject(PANO, 4, 8, CUBE, 12, 2, samples=-3) == BAD_SHAPE
    assert reproject(PANO, 4, 8, CUBE, 12, 2, samples=17) == BAD_SHAPE
    assert reproject(PANO, 1, 8, CUBE, 12, 2) == BAD_SHAPE and reproject(PANO, 4, 8, CUBE, 6, 1) == BAD_SHAPE
    assert reproject(PINHOLE, 1, 8, PANO, 4, 8) == BAD_SHAPE and reproject(FISHEYE, 4, 4, FISHEYE, 1, 4) == BAD_SHAPE
    assert reproject(PANO, 65536, 32768, CUBE, 12, 2) == BAD_SHAPE and reproject(PANO, 4, 8, PINHOLE, 32768, 65536) == BAD_SHAPE
    assert reproject(PANO, 4, 8, CUBE, 12, 2, N=0) == BAD_SHAPE and reproject(PANO, 4, 8, CUBE, 12, 2, C=0) == BAD_SHAPE
    assert reproject(7, 4, 8, CUBE, 12, 2) == UNSUPPORTED and reproject(PANO, 4, 8, -1, 12, 2) == UNSUPPORTED
    assert reproject(STEREO, 4, 8, PANO, 4, 8) == UNSUPPORTED and reproject(PANO, 4, 8, STEREO, 4, 8) == UNSUPPORTED
    torch.cuda.synchronize()
