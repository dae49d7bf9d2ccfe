"""The host-side conventions the path and probe renderers share (views._FrameSink, _put_groups, _render_rows, _probe_rig;
DESIGN.md 6r), on a small random-initialised model: every path function writes the frames it returns, whatever the frame
grouping, and one pass of the row loop serves light_probes, shadow_maps and probe_rgbd.  Everything is compared bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

import _volume_scenes as scenes

pytestmark = pytest.mark.gpu

H, W, N_POSES, CHUNK = 8, 16, 3, 50  # 128-ray frames in 50-ray chunks: a chunk straddles two frames


def dev():
    return torch.device("cuda:0")


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()


@functools.lru_cache(maxsize=None)
def model():
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    m = pn.PanoMipNeRF(num_samples=8, rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    m.mlp.load_state_dict(orc.init_params(4, 5))
    return m.to(dev())


def pose_at(p):
    m = np.eye(4)
    m[:3, 3] = p
    return m


def _poses():
    return np.stack([pose_at((0.0, 0.0, 0.0)), pose_at((0.1, 0.0, -0.1)), pose_at((0.15, 0.05, -0.2))])


def _render_path(out_dir):
    import pano_nerf_amd as pn
    from pano_nerf_amd import views
    return views.render_path(model(), views.pano_camera(H, W), _poses(), pn.generate_lit_rays(10, 0.01),
                             kinds=("ldr", "ldr_surf", "depth", "normal", "albedo", "hdr"), exposure=0.5, out_dir=out_dir,
                             chunk_rays=CHUNK)


def _render_path_warped(out_dir):
    from pano_nerf_amd import views
    return views.render_path_warped(model(), views.pano_camera(H, W), _poses(), 2, kinds=("ldr", "hdr", "depth"),
                                    exposure=0.5, out_dir=out_dir, chunk_rays=CHUNK)


def _relight_path(out_dir):
    import pano_nerf_amd as pn
    from pano_nerf_amd import relight as rl, views
    lights = [rl.PointLight((0.3, 0.4, -0.2), (3.0, 2.0, 1.0)),
              rl.PointLight((-0.4, 0.5, 0.3), 2.0, axis=(0.3, -1.0, -0.2), inner_deg=25.0, outer_deg=50.0)]
    return rl.relight_path(model(), views.pano_camera(H, W), _poses(), lights, pn.generate_lit_rays(10, 0.01),
                           map_size=(8, 16), kinds=("ldr", "hdr", "direct"), exposure=0.5, out_dir=out_dir, chunk_rays=CHUNK)


def _insert_path(out_dir):
    from pano_nerf_amd import objects, views
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32) * 0.12 + np.array([0, 0, -0.6], np.float32)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    obj = objects.VirtualObject(torch.from_numpy(v).to(dev()), torch.from_numpy(f).to(dev()))
    return objects.insert_path(model(), views.pano_camera(H, W), _poses(), obj, probe_size=(8, 16),
                               kinds=("ldr", "mask", "depth"), out_dir=out_dir, chunk_rays=CHUNK)


def _render_volume_path(out_dir):
    from pano_nerf_amd import views, volume
    data, bounds, deg, attrs = scenes.volume("checker")
    vol = volume.RadianceVolume(torch.from_numpy(data.copy()).to(dev()), bounds, deg, attrs)
    poses = np.stack([scenes.camera_pose()] * N_POSES)
    poses[1, :3, 3] += (0.05, 0.02, -0.03)
    poses[2, :3, 3] += (-0.04, 0.03, 0.06)
    return volume.render_volume_path(vol, views.pano_camera(H, W), poses, ("ldr", "depth", "hdr", "albedo", "normal"),
                                     scenes.CAMERA_NEAR, scenes.CAMERA_FAR, exposure=0.5, out_dir=out_dir)


PATHS = {"render_path": _render_path, "render_path_warped": _render_path_warped, "relight_path": _relight_path,
         "insert_path": _insert_path, "render_volume_path": _render_volume_path}


@pytest.mark.parametrize("name", sorted(PATHS))
def test_path_files_are_the_frames_in_any_grouping(name, tmp_path, monkeypatch):
    """Groups of two frames (so the last group of the three poses is short) against the default single group, and the
    files of out_dir against the frames in memory."""
    from pano_nerf_amd import io_exr, views
    run = PATHS[name]
    monkeypatch.setattr(views, "_PATH_GROUP_RAYS", 2 * H * W)
    frames = run(None)
    written = run(str(tmp_path))
    monkeypatch.undo()
    assert views._PATH_GROUP_RAYS >= N_POSES * H * W
    whole = run(None)
    # render_path_warped's coverage is the caller's: returned either way, and no frame kind
    extra = {"coverage"} if name == "render_path_warped" else set()
    assert set(written) == extra and set(whole) == set(frames)
    kinds = sorted(set(frames) - extra)
    assert kinds and sorted(os.listdir(tmp_path)) == kinds
    for k in sorted(frames):
        assert same_bits(frames[k], whole[k]), k
    for k in extra:
        assert tuple(frames[k].shape) == (N_POSES, H, W) and same_bits(frames[k], written[k])
    for k in kinds:
        hdr = k == "hdr"
        assert tuple(frames[k].shape) == (N_POSES, H, W, 3) and frames[k].dtype == (torch.float32 if hdr else torch.uint8)
        names = [f"{i:05d}.{'exr' if hdr else 'png'}" for i in range(N_POSES)]
        assert sorted(os.listdir(tmp_path / k)) == names, k
        for i, fname in enumerate(names):
            back = (io_exr.read_exr if hdr else io_exr.read_png)(str(tmp_path / k / fname))
            assert same_bits(torch.from_numpy(back), frames[k][i]), (k, i)
    assert any(bool(frames[k].any()) for k in kinds)


def test_one_row_pass_serves_every_probe_kind():
    """P H W = 144 rows in 50-row chunks: the chunk size does not divide them and a chunk crosses the probe boundary."""
    from pano_nerf_amd import emitters, lighting, relight as rl, views
    P, h, w = 2, 6, 12
    pos = torch.tensor([[0.3, 0.4, -0.2], [-0.4, 0.5, 0.3]], device=dev())
    rgb = torch.empty(P * h * w, 3, device=dev())
    dep = torch.empty(P * h * w, 1, device=dev())
    with torch.no_grad():
        rig = views._probe_rig(pos, views.pano_camera(h, w), dev())
        views._render_rows(model(), rig, 0, P * h * w, None, False, False, 0.0, 10.0, CHUNK,
                           {"fine_rgb": rgb, "fine_dep": dep}, streams=1)
    want_rgb, want_dep = rgb.view(P, h, w, 3).permute(0, 3, 1, 2), dep.view(P, h, w)
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(dep).all()) and float(rgb.abs().max()) > 0
    probes = lighting.light_probes(model(), pos, h, w, chunk_rays=CHUNK)
    assert same_bits(probes, want_rgb) and probes.permute(0, 2, 3, 1).is_contiguous()
    assert same_bits(rl.shadow_maps(model(), pos, h, w, chunk_rays=CHUNK), want_dep)
    both = emitters.probe_rgbd(model(), pos, h, w, chunk_rays=CHUNK)
    assert same_bits(both[0], want_rgb) and same_bits(both[1], want_dep) and both[0].permute(0, 2, 3, 1).is_contiguous()
    cube = rl.shadow_maps(model(), pos, kind="cube", width=4, chunk_rays=CHUNK)
    assert tuple(cube.shape) == (P, 24, 4)
    for p in range(P):
        view = views.render_view(model(), views.cubemap_camera(4), pose_at(pos[p].cpu().numpy().astype(np.float64)),
                                 outputs=("depth",))["fine_dep"]
        assert same_bits(cube[p], view[0, 0]), p
    none = pos[:0]
    assert tuple(lighting.light_probes(model(), none, h, w).shape) == (0, 3, h, w)
    assert tuple(rl.shadow_maps(model(), none, h, w).shape) == (0, h, w)
    assert tuple(rl.shadow_maps(model(), none, kind="cube", width=4).shape) == (0, 24, 4)
    assert [tuple(t.shape) for t in emitters.probe_rgbd(model(), none, h, w)] == [(0, 3, h, w), (0, h, w)]
