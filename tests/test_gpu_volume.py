"""The radiance volume on the device: pn_volume_march against the numpy restatement (tests/_volume_ref.py) to ONE fp32
ulp, jumps against no jumps bit for bit, the occupancy, the bake, and the image-level wrappers.

Tolerance (derived): both sides evaluate the same fp64 formulas in the same order and differ only through exp, by a few
fp64 ulps, i.e. 2^-29 of an fp32 ulp even after thousands of terms; every output is held to one fp32 ulp of the
restatement, plus 2^-40 of the restatement's sum of absolute terms for the signed attribute sums that cancel.  Rows the
restatement flags as fragile (a transmittance within 1e-9 of t_min, a sample within 1e-9 grid units of a box face) are
left out; tests/test_volume_cpu.py caps them at 1 % per scene.  The worst ulp of every comparison is printed."""
import functools

import numpy as np
import pytest
import torch

import _volume_ref as ref
import _volume_scenes as scenes

pytestmark = pytest.mark.gpu

SLACK = 2.0 ** -40


def dev():
    return torch.device("cuda:0")


def on_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())


@functools.lru_cache(maxsize=None)
def device_volume(name):
    from pano_nerf_amd import volume
    data, bounds, deg, attrs = scenes.volume(name)
    return volume.RadianceVolume(on_dev(data.copy()), bounds, deg, attrs)


@functools.lru_cache(maxsize=None)
def device_rays():
    return {k: on_dev(v) for k, v in scenes.rays().items()}


def big_step(name):
    data, bounds, _, _ = scenes.volume(name)
    return float(np.float32(2.7 * max(scenes.placement(bounds, data.shape[:3])[1])))


@functools.lru_cache(maxsize=None)
def reference(name, t_min, big):
    data, bounds, deg, _ = scenes.volume(name)
    lo, step = scenes.placement(bounds, data.shape[:3])
    ms = np.float32(big_step(name)) if big else scenes.march_step(bounds, data.shape[:3])
    r = scenes.rays()
    return ref.march(data, lo, step, deg, r["origins"], r["directions"], r["near"], r["far"], ms, t_min)


def compare(got, want, what, rows=slice(None)):
    """every output of march_rays against the restatement; returns the worst ulp"""
    keep = ~want["fragile"][rows]
    assert keep.mean() >= 0.99 or keep.size < 100, (what, int((~keep).sum()))
    worst = 0.0
    attrs = torch.cat([got[k] for k in got if k not in ("rgb", "depth", "acc")], 1) if len(got) > 3 else None
    pairs = [("rgb", got["rgb"], want["rgb"], want["abs_rgb"]), ("acc", got["acc"][:, 0], want["acc"], want["acc"]),
             ("depth", got["depth"][:, 0], want["depth"], want["abs_wt"] * 0.0)]
    if attrs is not None:
        pairs.append(("attrs", attrs, want["attrs"], want["abs_attrs"]))
    for name, g, w, a in pairs:
        g, w, a = g.cpu().numpy()[keep], w[rows][keep], a[rows][keep]
        assert np.array_equal(g == 0, w.astype(np.float32) == 0), (what, name, "zero outputs differ")
        u = ref.ulps(g, w, SLACK * a)
        worst = max(worst, float(u.max()) if u.size else 0.0)
        assert (u <= 1.0).all(), (what, name, float(u.max()))
    dead = ~want["marched"][rows]
    for k, v in got.items():
        assert not v.cpu().numpy()[dead].any(), (what, k, "an invalid row wrote something")
    return worst


def outputs_of(vol):
    return ("rgb", "depth", "acc") + vol.attribute_names


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("name", sorted(scenes.VOLUMES))
def test_march_matches_the_restatement(name):
    from pano_nerf_amd import volume
    vol, r = device_volume(name), device_rays()
    worst = 0.0
    for t_min in (0.0, 1e-3, 0.5):
        for big in (False, True):
            want = reference(name, t_min, big)
            for skip in (True, False):
                got = volume.march_rays(vol, r["origins"], r["directions"], r["near"], r["far"],
                                        big_step(name) if big else None, t_min, skip, outputs_of(vol))
                worst = max(worst, compare(got, want, (name, t_min, big, skip)))
    print(f"{name}: worst ulp {worst:.3f}")


@pytest.mark.parametrize("R", [0, 1, 63, 65, 130])
def test_row_counts(R):
    from pano_nerf_amd import volume
    vol, r = device_volume("partial"), device_rays()
    want = reference("partial", 1e-3, False)
    first = 7  # rows 7 .. 7 + R: valid and invalid rows of every kind
    got = volume.march_rays(vol, *[r[k][first:first + R] for k in ("origins", "directions", "near", "far")],
                            outputs=outputs_of(vol))
    assert got["rgb"].shape == (R, 3) and got["depth"].shape == (R, 1) and got["albedo"].shape == (R, 3)
    if R:
        print(f"R = {R}: worst ulp {compare(got, want, R, slice(first, first + R)):.3f}")


@pytest.mark.parametrize("camera", sorted(scenes.CAMERAS))
def test_camera_frames_match_the_restatement(camera):
    from pano_nerf_amd import views, volume
    ctor, args = scenes.CAMERAS[camera]
    rays = views.generate_camera_rays(getattr(views, ctor)(*args), scenes.camera_pose(), scenes.CAMERA_NEAR,
                                      scenes.CAMERA_FAR, dev())
    host = [x.cpu().numpy() for x in (rays.origins, rays.directions, rays.near, rays.far)]
    for name in ("checker", "partial"):
        data, bounds, deg, _ = scenes.volume(name)
        lo, step = scenes.placement(bounds, data.shape[:3])
        want = ref.march(data, lo, step, deg, *host, scenes.march_step(bounds, data.shape[:3]), 1e-3)
        vol = device_volume(name)
        for skip in (True, False):
            got = volume.march_rays(vol, rays.origins, rays.directions, rays.near, rays.far, skip=skip,
                                    outputs=outputs_of(vol))
            print(f"{camera} / {name} / skip={skip}: worst ulp {compare(got, want, (camera, name, skip)):.3f}")


# ----------------------------------------------------------------------------------------- 2. jumps change no bit
@pytest.mark.parametrize("name", sorted(scenes.VOLUMES))
def test_skip_is_bit_identical_and_deterministic(name):
    from pano_nerf_amd import volume
    vol, r = device_volume(name), device_rays()
    for step in (None, big_step(name)):
        for t_min in (0.0, 1e-3):
            runs = [volume.march_rays(vol, r["origins"], r["directions"], r["near"], r["far"], step, t_min, skip,
                                      outputs_of(vol)) for skip in (True, False, True)]
            for k in runs[0]:
                a, b, c = (x[k].view(torch.int32) for x in runs)
                assert torch.equal(a, b), (name, step, t_min, k, "skip changed bits")
                assert torch.equal(a, c), (name, step, t_min, k, "two calls differ")


def test_taps_count_the_samples():
    from pano_nerf_amd import volume
    vol, r = device_volume("checker"), device_rays()
    want = reference("checker", 1e-3, False)
    keep = ~want["fragile"]
    args = (vol, r["origins"], r["directions"], r["near"], r["far"], None, 1e-3)
    plain = volume.march_rays(*args, False, ("taps",))["taps"].cpu().numpy()
    jumped = volume.march_rays(*args, True, ("taps", "rgb"))["taps"].cpu().numpy()
    assert np.array_equal(plain[keep, 0], want["evaluated"][keep]) and np.array_equal(plain[keep, 1], want["hits"][keep])
    assert np.array_equal(jumped[:, 1], plain[:, 1]) and (jumped[:, 0] <= plain[:, 0]).all()
    assert jumped[:, 0].sum() < 0.7 * plain[:, 0].sum()


# --------------------------------------------------------------------------------------------------- 3. occupancy
@pytest.mark.parametrize("name", sorted(scenes.VOLUMES))
def test_occupancy_matches_numpy(name):
    vol = device_volume(name)
    want = ref.occupancy(scenes.volume(name)[0])
    assert vol.occupancy.dtype == torch.uint8 and tuple(vol.occupancy.shape) == want.shape
    assert np.array_equal(vol.occupancy.cpu().numpy(), want)


def test_refresh_after_an_edit():
    from pano_nerf_amd import volume
    data, bounds, deg, attrs = scenes.volume("single")
    vol = volume.RadianceVolume(on_dev(data.copy()), bounds, deg, attrs)
    assert int(vol.occupancy.sum()) == 1
    vol.sigma[3, 4, 8] = 2.0  # a vertex on the face between bricks (0, 0, 0) and (0, 0, 1)
    vol.sigma[16, 16, 16] = float("nan")
    assert int(vol.occupancy.sum()) == 1  # stale until refreshed
    edited = data.copy()
    edited[3, 4, 8, 0], edited[16, 16, 16, 0] = 2.0, np.nan
    assert np.array_equal(vol.refresh().occupancy.cpu().numpy(), ref.occupancy(edited))
    assert int(vol.occupancy.sum()) == 2 and int(vol.occupancy[1, 1, 1]) == 0


# -------------------------------------------------------------------------------------------------------- 4. bake
def make_model(cls):
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    extra = dict(mlp_num_density_channels=5, num_env_samples=10) if cls == "pano" else {}
    m = (pn.PanoMipNeRF if cls == "pano" else pn.MipNeRF)(num_samples=8, rgb_activation="softplus", **extra)
    m.mlp.load_state_dict(orc.init_params(4, 5 if cls == "pano" else 1))
    return m.to(dev())


@pytest.mark.parametrize("cls,attributes", [("pano", ("albedo", "normal")), ("mip", ("normal",)), ("mip", ())])
@pytest.mark.parametrize("resolution", [9, (6, 7, 10)])
def test_bake_volume(cls, attributes, resolution):
    from pano_nerf_amd import geometry, volume
    model = make_model(cls)
    bounds = ((-0.8, -0.6, -0.7), (0.7, 0.9, 0.6))
    sigma = geometry.density_grid(model, bounds, resolution)
    sigma_min = float(sigma.median())
    deg = 1 if cls == "pano" else 2
    K = (deg + 1) ** 2
    vol = volume.bake_volume(model, bounds, resolution, deg, sigma_min=sigma_min, attributes=attributes)
    keep = sigma > sigma_min
    M = int(keep.sum())
    assert 0 < M < sigma.numel()
    assert vol.sh_degree == deg and vol.attribute_names == attributes and vol.data.shape[3] == 1 + 3 * K + 3 * len(attributes)
    assert torch.equal(vol.sigma.view(torch.int32), torch.where(keep, sigma, 0.0).view(torch.int32))
    assert not vol.data[~keep].any()
    idx = torch.nonzero(keep.view(-1)).view(-1)
    step = geometry._placement(bounds, geometry._resolution(resolution))[1]
    var = max(step) ** 2 / 12.0
    pts = geometry.grid_points(bounds, resolution, 0.0, dev())[0][idx]
    if attributes:
        q = geometry.query_field(model, pts, var, outputs=attributes)
        for name in attributes:
            got = vol.attributes[name].reshape(-1, 3)[idx]
            assert torch.equal(got.view(torch.int32), q[name].view(torch.int32)), name
    dirs = volume.fibonacci_directions(4 * K).astype(np.float32)
    assert abs(np.linalg.norm(dirs, axis=1) - 1).max() < 1e-6
    P = np.linalg.pinv(volume.sh_basis(dirs.astype(np.float64), deg))
    want = np.zeros((M, K, 3))
    for i in range(dirs.shape[0]):
        rgb = geometry.query_field(model, pts, var, viewdirs=on_dev(dirs[i]), outputs=("rgb",))["rgb"]
        want = want + P[:, i][None, :, None] * rgb.cpu().numpy().astype(np.float64)[:, None, :]
    got = vol.coeff.reshape(-1, K, 3)[idx].cpu().numpy()
    u = ref.ulps(got, want)
    print(f"bake {cls} {resolution}: {M} of {sigma.numel()} vertices, worst coefficient ulp {u.max():.3f}")
    assert (u <= 1.0).all()


def test_bake_defaults():
    from pano_nerf_amd import geometry, volume
    model = make_model("pano")
    bounds = ((-0.8, -0.6, -0.7), (0.7, 0.9, 0.6))
    vol = volume.bake_volume(model, bounds, 5)
    sigma = geometry.density_grid(model, bounds, 5)
    diag = float(np.linalg.norm(np.array(bounds[1]) - np.array(bounds[0])))
    assert torch.equal(vol.sigma, torch.where(sigma > 0.01 / diag, sigma, 0.0))
    assert vol.sh_degree == 1 and vol.attribute_names == ("albedo", "normal")
    keep0 = volume.bake_volume(model, bounds, 5, 0, sigma_min=0.0, attributes=())
    assert torch.equal(keep0.sigma, torch.where(sigma > 0, sigma, 0.0)) and keep0.data.shape[3] == 4


# ---------------------------------------------------------------------------------------------------- 5-8. wrappers
@pytest.mark.parametrize("camera", sorted(scenes.CAMERAS))
def test_render_volume_is_march_rays_on_the_cameras_rays(camera):
    from pano_nerf_amd import views, volume
    ctor, args = scenes.CAMERAS[camera]
    cam = getattr(views, ctor)(*args)
    vol = device_volume("checker")
    pose = scenes.camera_pose()
    outs = outputs_of(vol)
    img = volume.render_volume(vol, cam, pose, outs, scenes.CAMERA_NEAR, scenes.CAMERA_FAR)
    rays = views.generate_camera_rays(cam, pose, scenes.CAMERA_NEAR, scenes.CAMERA_FAR, dev())
    rows = volume.march_rays(vol, rays.origins, rays.directions, rays.near, rays.far, outputs=outs)
    mask = on_dev(views.camera_mask(cam)).reshape(-1, 1)
    for k in outs:
        assert img[k].shape == (1, rows[k].shape[1], cam.h, cam.w)
        flat = img[k][0].permute(1, 2, 0).reshape(cam.h * cam.w, -1)
        assert torch.equal(flat, torch.where(mask, rows[k], 0.0)), (camera, k)
    if camera == "fisheye":
        assert not bool(mask.all()) and not img["acc"][0, 0][~mask.view(cam.h, cam.w)].any()
    assert float(img["acc"].max()) > 0.5


def test_render_volume_path_frames_are_to_frame_of_render_volume(tmp_path):
    from pano_nerf_amd import io_exr, views, volume
    vol = device_volume("checker")
    cam = views.perspective_camera(12, 16, 14.0)
    poses = np.stack([scenes.camera_pose(), scenes.camera_pose()])
    poses[1, :3, 3] += (0.05, 0.02, -0.03)
    kinds = ("ldr", "depth", "hdr", "albedo", "normal")
    frames = volume.render_volume_path(vol, cam, poses, kinds, scenes.CAMERA_NEAR, scenes.CAMERA_FAR)
    for i in range(2):
        img = volume.render_volume(vol, cam, poses[i], ("rgb", "depth", "albedo", "normal"), scenes.CAMERA_NEAR,
                                   scenes.CAMERA_FAR)
        assert torch.equal(frames["ldr"][i], views.to_frame(img["rgb"], "ldr"))
        assert torch.equal(frames["depth"][i], views.to_frame(img["depth"], "depth", scenes.CAMERA_NEAR, scenes.CAMERA_FAR))
        assert torch.equal(frames["hdr"][i], img["rgb"][0].permute(1, 2, 0))
        assert torch.equal(frames["albedo"][i], views.to_frame(img["albedo"], "albedo"))
        assert torch.equal(frames["normal"][i], views.to_frame(img["normal"], "normal"))
    assert volume.render_volume_path(vol, cam, poses, ("ldr", "hdr"), scenes.CAMERA_NEAR, scenes.CAMERA_FAR,
                                     out_dir=str(tmp_path)) == {}
    assert np.array_equal(io_exr.read_exr(str(tmp_path / "hdr" / "00001.exr")), frames["hdr"][1].cpu().numpy())
    assert (tmp_path / "ldr" / "00000.png").exists()
    with pytest.raises(ValueError):
        volume.render_volume_path(device_volume("one_brick"), cam, poses, ("albedo",))  # the volume has no albedo


def test_volume_probes_are_panorama_renders():
    from pano_nerf_amd import lighting, views, volume
    vol = device_volume("partial")
    pos = on_dev(np.array([[0.013, -0.021, 0.037], [0.3, 0.2, -0.9]], np.float32))
    probes = volume.volume_probes(vol, pos, 8, 16, 0.0, 2.5)
    assert probes.shape == (2, 3, 8, 16)
    for p in range(2):
        c2w = np.eye(4, dtype=np.float32)
        c2w[:3, 3] = pos[p].cpu().numpy()
        img = volume.render_volume(vol, views.pano_camera(8, 16), c2w, ("rgb",), 0.0, 2.5)["rgb"]
        assert torch.equal(probes[p], img[0])
    sh = lighting.sh_project(probes)
    assert sh.shape == (2, 9, 3) and bool(torch.isfinite(sh).all()) and float(sh[:, 0].abs().max()) > 0


def test_depth_feeds_fusion_and_warping_unchanged():
    from pano_nerf_amd import fusion, views, volume
    vol = device_volume("checker")
    cam = views.perspective_camera(12, 16, 14.0)
    pose = scenes.camera_pose()
    img = volume.render_volume(vol, cam, pose, ("rgb", "depth", "acc"), scenes.CAMERA_NEAR, scenes.CAMERA_FAR)
    tsdf = fusion.TSDFVolume(scenes.BOUNDS, 17, device=dev()).integrate(img["depth"], cam, pose[None],
                                                                       depth_max=0.98 * scenes.CAMERA_FAR)
    assert int(tsdf.observed().sum()) > 0
    other = pose.copy()
    other[:3, 3] += (0.04, 0.0, 0.02)
    warped = views.warp_view(img["rgb"], img["depth"], cam, pose, cam, other)
    assert warped["image"].shape == (1, 3, 12, 16) and float(warped["coverage"].mean()) > 0.5


# ------------------------------------------------------------------------------------------------------- 9. files
def test_save_and_load_bit_for_bit(tmp_path):
    from pano_nerf_amd import volume
    for name in ("nan", "strides"):
        vol = device_volume(name)
        vol.save(str(tmp_path / name))
        back = volume.RadianceVolume.load(str(tmp_path / name), dev())
        assert torch.equal(back.data.view(torch.int32), vol.data.view(torch.int32))
        assert back.bounds == vol.bounds and back.lo == vol.lo and back.step == vol.step
        assert back.sh_degree == vol.sh_degree and back.attribute_names == vol.attribute_names
        assert torch.equal(back.occupancy, vol.occupancy)


# ------------------------------------------------------------------------------------------------- 10. error paths
def test_error_paths():
    from pano_nerf_amd import volume
    data, bounds, deg, attrs = scenes.volume("strides")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        volume.RadianceVolume(torch.from_numpy(data.copy()), bounds, deg, attrs)
    with pytest.raises(ValueError, match="channels"):
        volume.RadianceVolume(on_dev(data.copy()), bounds, 2, attrs)
    with pytest.raises(ValueError):
        volume.RadianceVolume(on_dev(data[:1].copy()), bounds, deg, attrs)  # an axis with one vertex
    with pytest.raises(ValueError):
        volume.RadianceVolume(on_dev(data.copy()), bounds, 3, attrs)
    vol, r = device_volume("strides"), device_rays()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        volume.march_rays(vol, r["origins"].cpu(), r["directions"], r["near"], r["far"])
    with pytest.raises(ValueError, match="outputs"):
        volume.march_rays(vol, r["origins"], r["directions"], r["near"], r["far"], outputs=("rgb", "roughness"))
    with pytest.raises(ValueError, match="outputs"):
        volume.march_rays(device_volume("one_cell"), r["origins"], r["directions"], r["near"], r["far"], outputs=("albedo",))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        volume.volume_probes(vol, torch.zeros(1, 3))
    with pytest.raises(ValueError, match="albedo"):
        volume.bake_volume(make_model("mip"), bounds, 5)
    with pytest.raises(ValueError, match="unknown attributes"):
        volume.bake_volume(make_model("mip"), bounds, 5, attributes=("roughness",))
    one = volume.march_rays(vol, r["origins"][:5], r["directions"][:5], 0.0, 3.0, outputs=("normal",))
    assert list(one) == ["normal"] and one["normal"].shape == (5, 3)
