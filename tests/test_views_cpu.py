"""Novel views on the host (no GPU): camera paths against the reference's own outputs (gen_render_path,
create_spiral_poses, create_spheric_poses; tests/golden/make_views_golden.py), the Blender pinhole matrix against the
reference's camera_dirs, look_at, the jet table of the depth frames, and argument errors."""
import numpy as np
import pytest
import torch

from conftest import load_golden


def test_interpolate_path_is_gen_render_path():
    """float64 throughout, with a different Euler-extraction formula than scipy's: anything above 1e-9 is a bug."""
    from pano_nerf_amd import views
    g = load_golden("views_ref")
    got = views.interpolate_path(g["path/c2ws"], int(g["path/n_views"]))
    assert got.shape == g["path/interp"].shape == (40, 4, 4) and got.dtype == np.float64
    err = float(np.abs(got - g["path/interp"]).max())
    print("interpolate_path max |delta|", err)
    assert err <= 1e-9
    got7 = views.interpolate_path(g["path/c2ws"][:2], 7)
    assert got7.shape == g["path/interp7"].shape
    assert float(np.abs(got7 - g["path/interp7"]).max()) <= 1e-9
    # 3x4 poses are accepted as well
    assert float(np.abs(views.interpolate_path(g["path/c2ws"][:, :3], 30) - g["path/interp"]).max()) <= 1e-9


def test_spiral_and_spheric_paths():
    from pano_nerf_amd import views
    g = load_golden("views_ref")
    sp = views.spiral_path(g["spiral/radii"], float(g["spiral/focus_depth"]), 17)
    sh = views.spheric_path(float(g["spheric/radius"]), 13)
    for got, want in ((sp, g["spiral/poses"]), (sh, g["spheric/poses"])):
        assert got.shape == (want.shape[0], 4, 4)
        assert float(np.abs(got[:, :3, :] - want).max()) <= 1e-12
        assert np.array_equal(got[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (want.shape[0], 1)))


def test_perspective_camera_is_the_blender_camera():
    """The identity camera's directions in the golden are the reference's Blender camera_dirs.  The matrix form rounds
    1/f and w/(2f) to fp32 and evaluates (m0 x + m1 y) + m2 in fp32 (as the kernel does): a few fp32 roundings of terms no
    larger than |d|, so within 2 ulp of |d| (np.spacing of the fp32 norm, >= 2^-23 since |d_z| = 1) per component."""
    from pano_nerf_amd import views
    g = load_golden("views_ref")
    h, w = int(g["blender/h"]), int(g["blender/w"])
    cam = views.perspective_camera(h, w, focal=float(g["blender/focal"]))
    assert cam.h == h and cam.w == w and cam.pix2cam.dtype == np.float32 and cam.pix2cam.shape == (3, 3)
    m = cam.pix2cam
    x, y = np.meshgrid(np.arange(w, dtype=np.float32) + np.float32(0.5), np.arange(h, dtype=np.float32) + np.float32(0.5))
    got = np.stack([(m[k, 0] * x + m[k, 1] * y) + m[k, 2] for k in range(3)], -1)
    assert got.dtype == np.float32
    want = g["blender/directions"][2]  # c2w = identity
    ulp = np.spacing(np.linalg.norm(want, axis=-1).astype(np.float32)).astype(np.float64)[..., None]
    err = np.abs(got.astype(np.float64) - want) / ulp
    print("camera_dirs max error in ulp(|d|)", float(err.max()))
    assert float(err.max()) <= 2.0
    # the same camera from the field of view
    fov = np.degrees(0.9)
    cam2 = views.perspective_camera(h, w, fov_x_deg=fov)
    assert np.allclose(cam2.pix2cam, cam.pix2cam, rtol=1e-6, atol=0)
    # the Multicam form is taken as given
    p2c = g["multicam/pix2cam"]
    assert np.array_equal(views.perspective_camera(10, 14, pix2cam=p2c).pix2cam, p2c)


def test_look_at():
    from pano_nerf_amd import views
    rng = np.random.default_rng(3)
    for _ in range(20):
        eye, target = rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)
        c = views.look_at(eye, target)
        r = c[:3, :3]
        assert c.shape == (4, 4) and np.array_equal(c[3], [0, 0, 0, 1]) and np.array_equal(c[:3, 3], eye)
        assert np.abs(r.T @ r - np.eye(3)).max() < 1e-12
        assert abs(np.linalg.det(r) - 1.0) < 1e-12
        fwd = (target - eye) / np.linalg.norm(target - eye)
        assert np.abs(-r[:, 2] - fwd).max() < 1e-12
        assert abs(r[1, 0]) < 1e-12  # x stays horizontal for up = +y
    # it is create_spiral_poses' axis construction
    sp = views.spiral_path([0.5, 0.3, 0.2], 2.5, 5)
    for p in sp:
        assert np.abs(views.look_at(p[:3, 3], [0, 0, -2.5]) - p).max() < 1e-12


def test_jet_table_is_matplotlibs():
    from pano_nerf_amd import views
    g = load_golden("views_ref")
    assert views.JET_LUT.dtype == np.float32 and views.JET_LUT.shape == (256, 3)
    assert np.array_equal(views.JET_LUT, g["frames/jet_lut"])


def test_argument_errors():
    from pano_nerf_amd import views
    with pytest.raises(ValueError):
        views.perspective_camera(1, 8, focal=5.0)
    with pytest.raises(ValueError):
        views.perspective_camera(8, 1, focal=5.0)
    with pytest.raises(ValueError):
        views.perspective_camera(8, 8, focal=5.0, fov_x_deg=60.0)
    with pytest.raises(ValueError):
        views.perspective_camera(8, 8)
    with pytest.raises(ValueError):
        views.perspective_camera(8, 8, focal=5.0, pix2cam=np.eye(3))
    with pytest.raises(ValueError):
        views.perspective_camera(8, 8, pix2cam=np.eye(4))
    with pytest.raises(ValueError):
        views.perspective_camera(8, 8, focal=-1.0)
    with pytest.raises(ValueError):
        views.pano_camera(1, 8)
    cam = views.perspective_camera(8, 8, focal=5.0)
    for bad in (np.eye(3), np.zeros((4, 3)), np.zeros(16), np.full((4, 4), np.nan)):
        with pytest.raises(ValueError):
            views.generate_perspective_rays(cam, bad)
        with pytest.raises(ValueError):
            views.PerspectiveRayPool(cam, [bad])
    with pytest.raises(ValueError):
        views.interpolate_path(np.zeros((2, 3, 3)), 6)
    with pytest.raises(ValueError):
        views.interpolate_path(np.eye(4)[None], 2)
    with pytest.raises(ValueError):
        views.look_at([0, 0, 0], [0, 0, 0])
    with pytest.raises(ValueError):
        views.look_at([0, 0, 0], [0, 1, 0])
    with pytest.raises(ValueError):
        views.to_frame(torch.zeros(1, 3, 4, 4), "sepia")
    with pytest.raises(ValueError):
        views.to_frame(torch.zeros(1, 3, 4, 4), "depth", 0.0, 1.0)  # depth takes one channel


def test_cpu_tensors_raise():
    from pano_nerf_amd import views
    with pytest.raises(RuntimeError):
        views.to_frame(torch.zeros(1, 3, 4, 4), "ldr")
    with pytest.raises(RuntimeError):
        views.to_frame(torch.zeros(1, 1, 4, 4), "depth", 0.0, 1.0)
    with pytest.raises(RuntimeError):
        views.generate_perspective_rays(views.perspective_camera(8, 8, focal=5.0), np.eye(4), device="cpu")


def test_frame_sink_on_host_tensors(tmp_path):
    """The frame sink of the path renderers with a CPU device (no library call is involved): in memory it holds what was
    put, with out_dir the files decode to the same frames bit for bit and a permuted view writes its contiguous copy's
    bytes."""
    import os
    from pano_nerf_amd import io_exr, views
    n, H, W = 3, 2, 4
    kinds = ("ldr", "depth", "hdr")
    rng = np.random.default_rng(11)
    want = {k: (torch.from_numpy(rng.standard_normal((n, H, W, 3)).astype(np.float32)) if k == "hdr" else
                torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8))) for k in kinds}
    cpu = torch.device("cpu")
    sink = views._FrameSink(kinds, n, H, W, cpu)
    files = views._FrameSink(kinds, n, H, W, cpu, str(tmp_path / "a"))
    views_only = views._FrameSink(kinds, n, H, W, cpu, str(tmp_path / "b"))
    for i in range(n):
        for k in kinds:
            sink.put(k, i, want[k][i])
            files.put(k, i, want[k][i])
            chw = want[k][i].permute(2, 0, 1).contiguous()  # the same frame behind a [3, H, W] buffer
            assert not chw.permute(1, 2, 0).is_contiguous()
            views_only.put(k, i, chw.permute(1, 2, 0))
    assert sorted(sink.frames) == sorted(kinds)
    for k in kinds:
        assert sink.frames[k].dtype == (torch.float32 if k == "hdr" else torch.uint8)
        assert sink.frames[k].shape == (n, H, W, 3) and sink.frames[k].device == cpu
        assert torch.equal(sink.frames[k].view(torch.uint8), want[k].view(torch.uint8)), k
    assert files.frames == {} and views_only.frames == {}
    for k in kinds:
        ext = "exr" if k == "hdr" else "png"
        names = [f"{i:05d}.{ext}" for i in range(n)]
        assert sorted(os.listdir(tmp_path / "a" / k)) == names and sorted(os.listdir(tmp_path / "b" / k)) == names
        for i, name in enumerate(names):
            back = (io_exr.read_exr if k == "hdr" else io_exr.read_png)(str(tmp_path / "a" / k / name))
            assert back.dtype == want[k].numpy().dtype and back.tobytes() == want[k][i].numpy().tobytes(), (k, i)
            with open(tmp_path / "a" / k / name, "rb") as fa, open(tmp_path / "b" / k / name, "rb") as fb:
                assert fa.read() == fb.read(), (k, i)
