"""The numpy reference of views.warp_view (tests/_warp_ref.py) against analysis: identity, pure rotation, an analytic
room, occlusion, the footprint rule, and the bookkeeping of the margin the GPU test (tests/test_gpu_warp.py) relies on.
No GPU: this is the reference checked against what can be worked out by hand."""
import math

import numpy as np
import pytest

import _cameras_ref as cr
import _warp_ref as wr
from pano_nerf_amd import views


def _pose(seed, t=0.3):
    return wr._pose(np.random.default_rng(seed), t)


CAMERAS = {"pano": views.pano_camera(12, 24), "pinhole": views.perspective_camera(12, 16, fov_x_deg=70.0),
           "cube": views.cubemap_camera(4), "fisheye": views.fisheye_camera(16, 16, fov_deg=170.0)}


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_identity(name):
    """same camera, same pose, max_splat = 1: every valid source pixel lands in its own pixel"""
    cam = CAMERAS[name]
    rng = np.random.default_rng(3)
    H, W = cam.h, cam.w
    depth = rng.uniform(1, 4, (1, H, W)).astype(np.float32)
    depth.reshape(-1)[[5, 17, 40, 41]] = [np.nan, 0.0, -2.0, np.inf]
    image = rng.uniform(0, 1, (1, 3, H, W))
    pose = _pose(4)
    res = wr.warp(cam, pose, depth, cam, pose, max_splat=1)
    valid = np.isfinite(depth[0]) & (depth[0] > 0) & views.camera_mask(cam)
    assert valid.sum() > 0.5 * H * W
    want = np.where(valid, np.arange(H * W).reshape(H, W), -1)
    assert np.array_equal(res["index"][0], want)
    img, dep, cov = wr.resolve(res, image, cam, fill=-7.0)
    assert np.array_equal(img[0][:, valid], image[0][:, valid]) and (img[0][:, ~valid] == -7.0).all()
    assert np.array_equal(cov[0], valid.astype(float)) and np.isnan(dep[0][~valid]).all()
    # the fp32-rounded rotation is orthonormal to ~1e-7 only, which is what 1e-6 allows for
    assert np.abs(dep[0][valid] / depth[0][valid].astype(float) - 1).max() < 1e-6


def test_pure_rotation_is_nearest_pixel_reprojection():
    """panorama to panorama at one position.  (a) a turn by whole columns maps pixel centres onto pixel centres: the warp
    is _cameras_ref.reproject (whose bilinear fetch at a centre is that pixel).  (b) a general rotation: a destination
    pixel shows the nearest source pixel whose direction _cameras_ref projects into it - the lowest-indexed one, as the
    depth grows a little with the index - positions within 1e-6 px of a pixel border excluded."""
    cam = views.pano_camera(12, 24)
    H, W = cam.h, cam.w
    rng = np.random.default_rng(5)
    image = rng.uniform(0, 1, (1, 3, H, W))
    depth = (2.0 + 1e-3 * np.arange(H * W).reshape(1, H, W) / (H * W)).astype(np.float32)
    src = np.eye(4)
    # (a)
    dst = np.eye(4)
    dst[:3, :3] = cr.rotation_matrix([0, 1, 0], 5 * 2 * np.pi / W)
    res = wr.warp(cam, src, depth, cam, dst, max_splat=1)
    img, _, cov = wr.resolve(res, image, cam)
    want, _ = cr.reproject(image, cam, cam, rotation=dst[:3, :3])  # dst direction -> src direction: R_src^T R_dst
    assert (cov == 1).all() and np.abs(img - want).max() < 1e-6  # the fp32 rotation puts a centre 1e-7 px off
    # (b)
    dst[:3, :3] = cr.rotation_matrix([0.3, 1.0, -0.5], 0.7)
    res = wr.warp(cam, src, depth, cam, dst, max_splat=1)
    img, _, _ = wr.resolve(res, image, cam)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    d, _ = cr.pix_to_dir(cam, jj + 0.5, ii + 0.5)
    R = dst[:3, :3].astype(np.float32).astype(float)
    info = cr.dir_to_pix(cam, d @ R)  # R_dst^T d, per row vector
    px, py = info["px"].reshape(-1), info["py"].reshape(-1)
    near_border = (np.abs(px - np.round(px)) < 1e-6) | (np.abs(py - np.round(py)) < 1e-6)
    pix = (np.floor(py).astype(int) * W + np.floor(px).astype(int) % W)
    want_idx = np.full(H * W, -1)
    for n in range(H * W - 1, -1, -1):
        if py[n] < H:
            want_idx[pix[n]] = n
    touched = np.zeros(H * W, bool)
    touched[pix[near_border & (py < H)]] = True
    got = res["index"][0].reshape(-1)
    assert touched.mean() < 0.05
    assert np.array_equal(got[~touched], want_idx[~touched])
    hit = (got >= 0) & ~touched
    assert np.array_equal(img[0].reshape(3, -1)[:, hit], image[0].reshape(3, -1)[:, got[hit]])


def test_analytic_room():
    """A panorama at the centre of a sphere of radius R = 2 (depth 2 everywhere) seen from o = (0.3, 0.1, -0.2), c = |o|.

    Along a unit direction u from o the sphere lies at r(u) = -o.u + sqrt((o.u)^2 + R^2 - c^2), and turning u by a small
    angle changes r by at most |dr/dangle| <= c r / sqrt(R^2 - c^2) (differentiate; |d(o.u)/dangle| <= c) = 0.19 r.
    The point a pixel shows covers that pixel with a k x k splat, so its position is within k / 2 destination pixels of the
    pixel centre in both coordinates: an angle of at most sqrt(2) (k / 2) a_d (a panorama's column step is at most its row
    step a_d in angle).  k <= size + 1 with size = t a_s / (rho a_d), and here a_s = a_d (same camera) and t / rho <= R /
    (R - c) = 1.23: the angle is at most 0.71 (1.23 + 1) a_s = 1.58 a_s and the depth error at most 0.19 * 1.58 r a_s =
    0.30 r a_s: inside the bound asserted, one source pixel's angular step a_s times the depth."""
    cam = views.pano_camera(16, 32)
    H, W = cam.h, cam.w
    R_, o = 2.0, np.array([0.3, 0.1, -0.2])
    dst = np.eye(4)
    dst[:3, 3] = o
    depth = np.full((1, H, W), R_, np.float32)
    for max_splat in (1, 4):
        res = wr.warp(cam, np.eye(4), depth, cam, dst, max_splat=max_splat)
        _, dep, cov = wr.resolve(res, None, cam)
        jj, ii = np.meshgrid(np.arange(W), np.arange(H))
        u, _ = cr.pix_to_dir(cam, jj + 0.5, ii + 0.5)
        ou = u @ o
        want = -ou + np.sqrt(ou * ou + R_ * R_ - o @ o)
        hit = cov[0] > 0
        assert hit.mean() > (0.6 if max_splat == 1 else 0.9)  # the footprint is isotropic: pole rows keep holes
        a_s = 2 * math.sin(0.5 * math.pi / H)
        assert (np.abs(dep[0][hit] - want[hit]) <= a_s * want[hit]).all()


def test_occlusion():
    """two fronto-parallel planes in a pinhole pair, at depths 1 (the left half of the source image) and 3: after a
    sideways move every destination pixel both planes reach shows the near plane"""
    cam = views.perspective_camera(16, 24, fov_x_deg=60.0)
    H, W = cam.h, cam.w
    depth = np.full((1, H, W), 3.0, np.float32)  # a pinhole's t is along (x, y, -1): the distance of the plane
    depth[0, :, :W // 2] = 1.0
    dst = np.eye(4)
    dst[:3, 3] = (-0.25, 0.0, 0.0)  # moving left moves the near plane right by more than the far one: it covers it
    res = wr.warp(cam, np.eye(4), depth, cam, dst, max_splat=2, margin=0.0)  # margin 0: the exact candidate sets
    near = (depth[0] == 1.0).reshape(-1)
    cover = res["wide"][0]
    assert np.array_equal(cover, res["shrunk"][0])
    both = cover[:, near].any(-1) & cover[:, ~near].any(-1)
    assert both.sum() >= 2 * H
    got = res["index"][0].reshape(-1)
    assert near[got[both]].all()
    only_far = cover[:, ~near].any(-1) & ~cover[:, near].any(-1)
    assert only_far.any() and (~near[got[only_far]]).all()


def test_footprint_closes_the_holes_of_a_magnified_plane():
    """a pinhole camera moves forward until a plane doubles in size (depth 2 -> 1): points land two pixels apart, so
    k = 1 leaves holes in the plane's image (3 of 4 pixels) and the footprint rule (size = 2) leaves none.  The plane
    fills a central window only, so that its doubled image stays in the frame, and the move has a small sideways part so
    that no position falls on a pixel border."""
    cam = views.perspective_camera(15, 15, fov_x_deg=70.0)
    depth = np.full((1, 15, 15), np.nan, np.float32)
    depth[0, 4:10, 4:10] = 2.0
    dst = np.eye(4)
    dst[:3, 3] = (0.013, 0.017, -1.0)
    holes = {}
    for max_splat in (1, 2):
        res = wr.warp(cam, np.eye(4), depth, cam, dst, max_splat=max_splat)
        ok = res["valid"][0]
        # about 2 on the axis; off it the angular measure grows with cos(theta_s) / cos(theta_d) > 1 (it ignores the slant)
        assert ok.sum() == 36 and res["size"][0][ok].min() > 1.9 and res["size"][0][ok].max() < 2.3
        idx = res["index"][0]
        ys, xs = np.where(idx >= 0)
        box = idx[ys.min():ys.max() + 1, xs.min():xs.max() + 1]
        assert box.shape[0] >= 11 and box.shape[1] >= 11
        holes[max_splat] = (box < 0).mean()
    assert holes[1] > 0.2
    assert holes[2] == 0.0


@pytest.mark.parametrize("max_splat", wr.SPLATS)
@pytest.mark.parametrize("scene", wr.SCENES, ids=[s["name"] for s in wr.SCENES])
def test_margin_bookkeeping(scene, max_splat):
    """A condition on the choice of scenes, not a measurement: at m = 1e-3 px the reference itself may call at most 10 %
    of a scene's destination pixels fragile (widened and shrunk candidate sets differ, or the two smallest rho within
    1e-5 relative); the estimate is ~6 m per source point times 4 - 9 candidates per pixel = 2 - 5 %, plus, where source 0
    is seen from its own pose, its pixels that land exactly on a border.  The scenes also have to exercise what they are
    there for: holes, hits, invalid depths and (pinhole destinations) points that do not project."""
    res = wr.reference(scene, max_splat)
    share = wr.fragile(res).mean()
    print(scene["name"], max_splat, "fragile share", share)
    assert share <= 0.10
    assert (res["index"] >= 0).mean() > 0.1
    assert not np.isfinite(scene["depth"]).all() and (scene["depth"][np.isfinite(scene["depth"])] <= 0).any()
    assert np.abs(scene["dst_c2ws"][:, None, :3, 3] - scene["src_c2ws"][None, :, :3, 3]).max() <= 0.5
    assert np.array_equal(scene["dst_c2ws"][0], scene["src_c2ws"][0])
    if cr.kind(scene["dst"]) == "pinhole":
        assert (~res["valid"]).mean() > 0.3
