"""Novel views on the GPU: pinhole rays against the reference's Blender and Multicam rays, the ray pool against the
generated rays bit for bit, frames against the reference's bytes, render_view against the renderer bit for bit,
render_path against per-frame render_view + to_frame, the files render_path writes, and argument errors."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

MODES = ("fused_f16x2", "fused_f16x2_t32", "fused", "fused_bf16", "layerwise")
U = 2.0 ** -24


def dev():
    return torch.device("cuda:0")


def make_model(cls, mode, **kw):
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    extra = dict(mlp_num_density_channels=5, num_env_samples=10) if cls == "pano" else {}
    model = (pn.PanoMipNeRF if cls == "pano" else pn.MipNeRF)(num_samples=16, rgb_activation="softplus", **extra, **kw)
    model.mlp.load_state_dict(orc.init_params(4, 5 if cls == "pano" else 1))
    model = model.to(dev())
    model.mlp_mode = mode
    return model


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype == torch.uint8:
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------- rays
def check_rays(rays, g, prefix, k, near, far):
    """Tolerances with u = 2^-24 from two 3-term fp32 dot products on each side: directions 16 u |d| per component,
    viewdirs 24 u, radii 24 u max |d| (a difference of neighbours doubles the direction error; 2 / sqrt(12) ~ 0.58);
    origins, lossmult, near and far exact."""
    H, W = int(g[prefix + "h"]), int(g[prefix + "w"])
    got = {f: getattr(rays, f).cpu().numpy().astype(np.float64).reshape(H, W, -1) for f in rays._fields}
    want = {f: g[prefix + f][k].astype(np.float64) for f in ("origins", "directions", "viewdirs", "radii", "lossmult")}
    nd = np.linalg.norm(want["directions"], axis=-1, keepdims=True)
    ed = float((np.abs(got["directions"] - want["directions"]) / nd).max()) / U
    ev = float(np.abs(got["viewdirs"] - want["viewdirs"]).max()) / U
    er = float(np.abs(got["radii"] - want["radii"]).max()) / (U * float(nd.max()))
    print(f"{prefix}{k}: directions {ed:.2f} u|d|, viewdirs {ev:.2f} u, radii {er:.2f} u max|d|")
    assert ed <= 16 and ev <= 24 and er <= 24
    assert np.array_equal(got["origins"], want["origins"])
    assert np.array_equal(got["lossmult"], want["lossmult"])
    assert np.array_equal(got["near"], np.full((H, W, 1), np.float32(near), np.float64))
    assert np.array_equal(got["far"], np.full((H, W, 1), np.float32(far), np.float64))
    assert not got["noise_var"].any()


def test_blender_rays_match_the_reference():
    from pano_nerf_amd import views
    g = load_golden("views_ref")
    cam = views.perspective_camera(int(g["blender/h"]), int(g["blender/w"]), focal=float(g["blender/focal"]))
    for k in range(3):  # two poses and the identity
        rays = views.generate_perspective_rays(cam, g["blender/c2ws"][k], 0.0, 10.0)
        assert rays.origins.shape == (cam.h * cam.w, 3) and rays.radii.shape == (cam.h * cam.w, 1)
        check_rays(rays, g, "blender/", k, 0.0, 10.0)


def test_multicam_rays_match_the_reference():
    from pano_nerf_amd import views
    g = load_golden("views_ref")
    cam = views.perspective_camera(int(g["multicam/h"]), int(g["multicam/w"]), pix2cam=g["multicam/pix2cam"])
    near, far = (float(v) for v in g["multicam/near_far"])
    rays = views.generate_perspective_rays(cam, g["multicam/c2w"], near, far)
    check_rays(rays, g, "multicam/", 0, near, far)


def test_pool_is_the_generated_rays():
    from pano_nerf_amd import views
    H, W = 9, 13
    cam = views.perspective_camera(H, W, fov_x_deg=55.0)
    rng = np.random.default_rng(4)
    c2ws = [views.look_at(rng.uniform(-2, 2, 3), rng.uniform(-0.5, 0.5, 3)).astype(np.float32) for _ in range(3)]
    images = [rng.random((H, W, 3)).astype(np.float32) for _ in range(3)]
    pool = views.PerspectiveRayPool(cam, c2ws, images, near=0.2, far=7.0)
    assert len(pool) == 3 * H * W
    full = [views.generate_perspective_rays(cam, c, 0.2, 7.0) for c in c2ws]
    allr = views.Rays(*[torch.cat([getattr(r, f) for r in full], 0) for f in views.Rays._fields])
    allrgb = torch.from_numpy(np.concatenate([im.reshape(-1, 3) for im in images], 0))
    last = [c * H * W + p for c in range(3) for p in ((H - 1) * W, (H - 1) * W + W - 1, W - 1, H * W - 1, (H - 2) * W + 3)]
    idx = torch.cat([torch.randint(0, len(pool), (500,), generator=torch.Generator().manual_seed(5)),
                     torch.tensor(last)]).to(dev())
    rays, rgb = pool.take(idx)
    for f in views.Rays._fields:
        assert bits_equal(getattr(rays, f), getattr(allr, f)[idx]), f
    assert bits_equal(rgb, allrgb.to(dev())[idx])
    pr = pool.rays
    for f in views.Rays._fields:
        assert bits_equal(getattr(pr, f), getattr(allr, f)), f
    r2, c2 = pool.sample(64, generator=torch.Generator(device=dev()).manual_seed(1))
    assert r2.origins.shape == (64, 3) and c2.shape == (64, 3)
    nopool = views.PerspectiveRayPool(cam, c2ws, near=0.2, far=7.0)
    r3, c3 = nopool.take(idx)
    assert c3 is None and bits_equal(r3.radii, allr.radii[idx])


# ----------------------------------------------------------------------------------------------------------- frames
def _k_bytes():
    """byte of each k = 0..255 through hdr_to_ldr(dtype='uint8') and save_results, in torch fp32 on the host"""
    k = torch.arange(256, dtype=torch.uint8)
    v = (k / 255.) ** (1 / 2.2)
    return (v.numpy() * 255).astype(np.uint8)


def _loose_compare(got, want, kind):
    """at most 1e-3 of the pixel-channels differ, by one byte each; for "ldr" a mismatch must be one step of k"""
    d = got.astype(np.int32) - want.astype(np.int32)
    n = int((d != 0).sum())
    print(f"{kind}: {n} of {d.size} pixel-channels differ ({n / d.size:.2e}), max |diff| {int(np.abs(d).max())}")
    assert np.abs(d).max() <= 1
    assert n <= 1e-3 * d.size
    if kind == "ldr" and n:
        kb = _k_bytes()
        for gb, wb in zip(got[d != 0], want[d != 0]):
            ks = np.nonzero(kb == wb)[0]
            assert any((k + s) in range(256) and kb[k + s] == gb for k in ks for s in (-1, 1)), (gb, wb)


def test_frames_match_the_reference_bytes():
    from pano_nerf_amd import views
    g = load_golden("views_ref")
    hdr = torch.from_numpy(g["frames/hdr"]).to(dev())
    for kind in ("ldr", "ldr_gt"):
        got = views.to_frame(hdr, kind)
        assert got.dtype == torch.uint8 and got.shape == (64, 96, 3) and got.device.type == "cuda"
        _loose_compare(got.cpu().numpy(), g["frames/" + kind], kind)
    nrm = views.to_frame(torch.from_numpy(g["frames/normal"]).to(dev()), "normal")
    _loose_compare(nrm.cpu().numpy(), g["frames/normal_frame"], "normal")
    alb = views.to_frame(torch.from_numpy(g["frames/albedo"]).to(dev()), "albedo")
    assert np.array_equal(alb.cpu().numpy(), g["frames/albedo_frame"])
    near, far = float(g["frames/near"]), float(g["frames/far"])
    depth = torch.from_numpy(g["frames/depth"]).to(dev())
    dep = views.to_frame(depth, "depth", near, far)
    mism = int((dep.cpu().numpy() != g["frames/depth_frame"]).sum())
    print("depth: mismatching bytes", mism)
    assert mism == 0
    # the under-range branch is covered: some shifted values lie below 0 (and some above 1)
    t = (g["frames/depth"] - np.float32(near)) / np.float32(far - near)
    x = t - t.min() / (t.max() - t.min())
    assert x.dtype == np.float32 and (x < 0).any() and (x > 1).any()
    assert bits_equal(dep, views.to_frame(depth, "depth", near, far))  # repeated calls: the same bytes
    dn = depth.clone()
    dn[0, 0, 5, 7] = float("nan")
    black = views.to_frame(dn, "depth", near, far).cpu().numpy()
    assert not black.any() and np.array_equal(black, g["frames/depth_nan_frame"])


def test_frames_exposure_and_strides():
    from pano_nerf_amd import views
    g = load_golden("views_ref")
    hdr = torch.from_numpy(g["frames/hdr"]).to(dev())
    assert bits_equal(views.to_frame(hdr, "ldr", exposure=0.0), views.to_frame(hdr, "ldr"))
    for kind in ("ldr", "ldr_gt"):
        assert bits_equal(views.to_frame(hdr, kind, exposure=1.0), views.to_frame(2 * hdr, kind))
    # a [1, 3, H, W] view of an [H, W, 3] buffer (how render_image returns images) reads in place
    hwc = hdr[0].permute(1, 2, 0).contiguous()
    view = hwc[None].permute(0, 3, 1, 2)
    assert bits_equal(views.to_frame(view, "ldr"), views.to_frame(hdr, "ldr"))
    nrm = torch.from_numpy(g["frames/normal"]).to(dev())
    assert bits_equal(views.to_frame(nrm[0].permute(1, 2, 0).contiguous()[None].permute(0, 3, 1, 2), "normal"),
                      views.to_frame(nrm, "normal"))


# ------------------------------------------------------------------------------------------------------- rendering
def _image(pn, model, rays, env, H, W):
    return pn.render_image(model, pn.Rays(*[x.view(1, H, W, -1) for x in rays]), env, H, W)


@pytest.mark.parametrize("mode", MODES)
def test_render_view_is_the_renderer(mode):
    import pano_nerf_amd as pn
    from pano_nerf_amd import views
    H, W = 12, 20
    model = make_model("pano", mode)
    cam = views.perspective_camera(H, W, fov_x_deg=70.0)
    c2w = views.look_at([0.3, 0.2, 1.2], [0.0, 0.0, 0.0])
    rays = views.generate_perspective_rays(cam, c2w)
    env = pn.generate_lit_rays(10, 0.01)
    img = dict(zip(("coarse_rgb", "fine_rgb", "coarse_dep", "fine_dep", "fine_nor", "albedo", "roughness", "surface_rgb",
                    "shading"), _image(pn, model, rays, env, H, W)))
    a = views.render_view(model, cam, c2w, outputs=("rgb", "depth"))
    assert sorted(a) == ["coarse_dep", "coarse_rgb", "fine_dep", "fine_rgb"]
    b = views.render_view(model, cam, c2w, outputs=("normal",))
    c = views.render_view(model, cam, c2w, env, outputs=("albedo", "surface", "shading"), chunk_rays=77)
    for out in (a, b, c):
        for k, v in out.items():
            assert v.shape == img[k].shape, k
            assert bits_equal(v, img[k]), (mode, k)
    # the panorama camera: pn_sample_pano_rays, the rays of generate_pano_rays
    pc2w = np.eye(4, dtype=np.float32)
    pc2w[:3, 3] = (0.1, -0.2, 0.3)
    prays = pn.generate_pano_rays(8, 16, pc2w)
    pimg = _image(pn, model, prays, env, 8, 16)
    p = views.render_view(model, views.pano_camera(8, 16), pc2w, env, outputs=("rgb", "normal", "shading"))
    assert bits_equal(p["fine_rgb"], pimg[1]) and bits_equal(p["fine_nor"], pimg[4]) and bits_equal(p["shading"], pimg[8])


@pytest.mark.parametrize("mode", MODES)
def test_render_view_mipnerf(mode):
    from pano_nerf_amd import views
    H, W = 10, 16
    model = make_model("mip", mode)
    cam = views.perspective_camera(H, W, focal=14.0)
    c2w = views.look_at([-0.4, 0.3, 1.0], [0.0, 0.1, 0.0])
    rays = views.generate_perspective_rays(cam, c2w)
    with torch.no_grad():
        (c_rgb, c_dep, *_), (f_rgb, f_dep, _, f_nor) = model(rays=rays, randomized=False, white_bkgd=False,
                                                             use_ort_loss=True)
    v = views.render_view(model, cam, c2w, outputs=("rgb", "depth", "normal"))
    img = lambda x: x.reshape(1, H, W, -1).permute(0, 3, 1, 2)
    for k, want in (("coarse_rgb", c_rgb), ("fine_rgb", f_rgb), ("coarse_dep", c_dep), ("fine_dep", f_dep),
                    ("fine_nor", f_nor)):
        assert bits_equal(v[k], img(want)), (mode, k)


def _path(n):
    from pano_nerf_amd import views
    rng = np.random.default_rng(9)
    return np.stack([views.look_at(rng.uniform(-1.5, 1.5, 3) + np.array([0, 0, 2.0]), [0, 0, 0]) for _ in range(n)])


def test_render_path_is_per_frame_render_view():
    import pano_nerf_amd as pn
    from pano_nerf_amd import views
    H, W, n = 24, 32, 5
    model = make_model("pano", "fused_f16x2")
    env = pn.generate_lit_rays(10, 0.01)
    cam = views.perspective_camera(H, W, fov_x_deg=60.0)
    poses = _path(n)
    kinds = ("ldr", "ldr_surf", "depth", "normal", "albedo", "hdr")
    # 2000-ray chunks: several frames of 768 rays per chunk, chunks crossing frame boundaries
    fr = views.render_path(model, cam, poses, env, kinds=kinds, near=0.0, far=10.0, exposure=0.5, chunk_rays=2000)
    assert sorted(fr) == sorted(kinds)
    for k in kinds:
        assert fr[k].shape == (n, H, W, 3) and fr[k].dtype == (torch.float32 if k == "hdr" else torch.uint8)
    for i in range(n):
        v = views.render_view(model, cam, poses[i], env, outputs=("rgb", "depth", "normal", "albedo", "surface"))
        assert bits_equal(fr["hdr"][i], v["fine_rgb"][0].permute(1, 2, 0)), i
        assert bits_equal(fr["ldr"][i], views.to_frame(v["fine_rgb"], "ldr", exposure=0.5)), i
        assert bits_equal(fr["ldr_surf"][i], views.to_frame(v["surface_rgb"], "ldr", exposure=0.5)), i
        assert bits_equal(fr["depth"][i], views.to_frame(v["fine_dep"], "depth", 0.0, 10.0)), i
        assert bits_equal(fr["normal"][i], views.to_frame(v["fine_nor"], "normal")), i
        assert bits_equal(fr["albedo"][i], views.to_frame(v["albedo"], "albedo")), i


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


def test_render_path_writes_files(tmp_path):
    from pano_nerf_amd import io_exr, views
    H, W, n = 24, 32, 3
    model = make_model("pano", "fused_f16x2")
    cam = views.perspective_camera(H, W, fov_x_deg=60.0)
    poses = _path(n)
    kinds = ("ldr", "depth", "normal", "hdr")
    fr = views.render_path(model, cam, poses, kinds=kinds, chunk_rays=1000)
    res = views.render_path(model, cam, poses, kinds=kinds, chunk_rays=1000, out_dir=str(tmp_path))
    assert res == {}
    for k in kinds:
        names = sorted(os.listdir(tmp_path / k))
        ext = "exr" if k == "hdr" else "png"
        assert names == [f"{i:05d}.{ext}" for i in range(n)], (k, names)
        for i in range(n):
            if k == "hdr":
                back = io_exr.read_exr(str(tmp_path / k / names[i]))
                assert np.array_equal(back, fr[k][i].cpu().numpy())
            else:
                assert np.array_equal(_read_png(str(tmp_path / k / names[i])), fr[k][i].cpu().numpy()), (k, i)


def test_bad_input_raises():
    import pano_nerf_amd as pn
    from pano_nerf_amd import views
    pano = make_model("pano", "fused_f16x2")
    mip = make_model("mip", "fused_f16x2")
    cam = views.perspective_camera(8, 8, focal=6.0)
    env = pn.generate_lit_rays(10, 0.01)
    with pytest.raises(RuntimeError):
        views.to_frame(torch.zeros(1, 3, 4, 4), "ldr")
    with pytest.raises(RuntimeError):
        views.generate_perspective_rays(cam, np.eye(4), device="cpu")
    with pytest.raises(ValueError):
        views.render_view(pano, cam, np.eye(4), outputs=("albedo",))  # no env_rays
    with pytest.raises(ValueError):
        views.render_view(mip, cam, np.eye(4), env, outputs=("shading",))  # MipNeRF has no surface outputs
    with pytest.raises(ValueError):
        views.render_path(mip, cam, _path(2), env, kinds=("ldr_surf",))
    with pytest.raises(ValueError):
        views.render_path(pano, cam, _path(2), kinds=("albedo",))
    with pytest.raises(ValueError):
        views.render_view(pano, cam, np.eye(4), outputs=("colour",))
    with pytest.raises(ValueError):
        views.to_frame(torch.zeros(1, 3, 4, 4, device=dev()), "depth", 0.0, 1.0)
    with pytest.raises(ValueError):
        views.to_frame(torch.zeros(1, 1, 4, 4, device=dev()), "depth")
