"""CPU checks of the camera models and of the reprojection statement (tests/_cameras_ref.py, fp64 numpy): round trips,
the cube map's edges and solid angles, the stereo panorama's geometry, reprojection identities, the orientation of the
cube-map convention end to end against the panorama quadrature, and constructor validation.  No GPU."""
import math

import numpy as np
import pytest

import _cameras_ref as ref
from pano_nerf_amd import views


def central_cameras():
    return [views.pano_camera(8, 16), views.perspective_camera(6, 8, fov_x_deg=90.0), views.cubemap_camera(4),
            views.fisheye_camera(9, 9, fov_deg=220.0)]


# --------------------------------------------------------------------------------------------------------- round trips
@pytest.mark.parametrize("cam", central_cameras() + [views.fisheye_camera(4, 4, fov_deg=360.0),
                                                     views.perspective_camera(5, 7, focal=4.0)], ids=lambda c: ref.kind(c))
def test_pixel_direction_pixel_round_trip(cam):
    """to 1e-9 px in fp64.  (The pinholes have matrices whose inverse is exact in fp32: cam2pix reaches the device rounded
    to fp32, and the statement rounds it the same way.)"""
    rng = np.random.default_rng(1)
    px, py = rng.uniform(0.01, cam.w - 0.01, 4000), rng.uniform(0.01, cam.h - 0.01, 4000)
    d, ok = ref.pix_to_dir(cam, px, py)
    if ref.kind(cam) == "fisheye":  # stay off the point antipodal to the axis, where every heading meets
        ok &= np.hypot(px - cam.w / 2, py - cam.h / 2) / cam.focal < math.pi - 1e-3
    assert ok.sum() > 1000
    # any positive scale of the direction projects to the same pixel
    back = ref.dir_to_pix(cam, d * rng.uniform(0.5, 2.0, (4000, 1)))
    assert back["valid"][ok].all()
    by = back["py"] + (back["face"] * cam.w if ref.kind(cam) == "cube" else 0)
    err = max(np.abs(back["px"] - px)[ok].max(), np.abs(by - py)[ok].max())
    print(ref.kind(cam), "round trip error (px)", err)
    assert err <= 1e-9


# ---------------------------------------------------------------------------------------------------------- cube map
def _edges(n=5):
    """the 24 face edges as [n, 3] unit points, each from one end to the other"""
    u = np.linspace(-1.0, 1.0, n)
    edges = {}
    for f in range(6):
        face = np.full(n, f)
        for name, (s, t) in dict(top=(u, -np.ones(n)), bottom=(u, np.ones(n)), left=(-np.ones(n), u),
                                 right=(np.ones(n), u)).items():
            d = ref.cube_table(face, s, t)
            edges[(f, name)] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return edges


def test_cube_edges_pair_up_one_to_one():
    edges = _edges()
    assert len(edges) == 24
    for key, e in edges.items():
        twins = [k for k, o in edges.items() if k != key
                 and (np.abs(o - e).max() < 1e-12 or np.abs(o[::-1] - e).max() < 1e-12)]
        assert len(twins) == 1 and twins[0][0] != key[0], (key, twins)


def test_cube_faces_cover_the_sphere_once():
    """every direction has exactly one (face, s, t) and the table maps it back: the inverse of the table is its inverse"""
    rng = np.random.default_rng(2)
    d = rng.normal(size=(5000, 3))
    cam = views.cubemap_camera(5)
    p = ref.dir_to_pix(cam, d)
    back, face = ref.cube_dir(5, p["px"], p["py"] + p["face"] * 5)
    assert np.array_equal(face, p["face"])
    back = back / np.linalg.norm(back, axis=-1, keepdims=True)
    assert np.abs(back - d / np.linalg.norm(d, axis=-1, keepdims=True)).max() < 1e-12
    # the axes themselves land in the middle of their faces, in the strip's order
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], float)
    q = ref.dir_to_pix(cam, axes)
    assert list(q["face"]) == [0, 1, 2, 3, 4, 5] and np.allclose(q["px"], 2.5) and np.allclose(q["py"], 2.5)
    # ties go to the earlier face
    ties = np.array([[1, 1, 0], [1, -1, 1], [-1, 0, 1], [0, 1, 1], [0, -1, -1], [1, 1, 1]], float)
    assert list(ref.dir_to_pix(cam, ties)["face"]) == [0, 0, 1, 2, 3, 0]


@pytest.mark.parametrize("size", [2, 3, 16])
def test_cube_solid_angles(size):
    w = views.cube_solid_angles(size)
    assert w.shape == (6 * size, size) and w.dtype == np.float64 and (w > 0).all()
    assert abs(w.sum() - 4 * math.pi) <= 1e-12
    faces = w.reshape(6, size, size)
    for f in faces:
        assert np.abs(f - faces[0]).max() <= 1e-15
        for g in (f.T, f[::-1], f[:, ::-1]):
            assert np.abs(g - f).max() <= 1e-15
    # against the integral of 1 / (x^2 + y^2 + 1)^(3/2) over one texel, by a fine midpoint rule
    n = 400
    e = 2.0 * np.arange(size + 1) / size - 1.0
    x = e[0] + (np.arange(n) + 0.5) / n * (e[1] - e[0])
    xx, yy = np.meshgrid(x, x)
    num = ((xx * xx + yy * yy + 1.0) ** -1.5).sum() * ((e[1] - e[0]) / n) ** 2
    assert abs(num - w[0, 0]) <= 1e-5 * w[0, 0]


def test_cube_faces_view():
    x = np.arange(2 * 3 * 12 * 2).reshape(2, 3, 12, 2)
    f = views.cube_faces(x)
    assert f.shape == (2, 6, 3, 2, 2)
    for k in range(6):
        assert np.array_equal(f[:, k], x[:, :, 2 * k:2 * k + 2])
    import torch
    ft = views.cube_faces(torch.from_numpy(x))
    assert np.array_equal(ft.numpy(), f)
    with pytest.raises(ValueError):
        views.cube_faces(np.zeros((3, 10, 2)))


def test_camera_mask():
    cam = views.fisheye_camera(5, 7, fov_deg=180.0)
    m = views.camera_mask(cam)
    assert m.shape == (5, 7) and m.dtype == bool
    u, v = np.meshgrid(np.arange(7) - 3.0, np.arange(5) - 2.0)
    assert np.array_equal(m, np.hypot(u, v) <= 2.5)
    assert np.array_equal(m, ref.rays(cam, np.eye(4))["lossmult"].reshape(5, 7) > 0)
    assert views.camera_mask(views.fisheye_camera(4, 4, fov_deg=360.0)).sum() == 12  # the corners lie beyond theta = pi
    for cam in (views.pano_camera(4, 8), views.cubemap_camera(2), views.perspective_camera(4, 4, focal=2.0),
                views.stereo_pano_camera(4, 8, 0.06, "left")):
        assert views.camera_mask(cam).all() and views.camera_mask(cam).shape == (cam.h, cam.w)


# ----------------------------------------------------------------------------------------------------- stereo panorama
def test_stereo_pano_geometry():
    H, W, ipd = 4, 8, 0.064
    c2w = np.eye(4)
    c2w[:3, :3] = ref.rotation_matrix((0.2, 0.9, -0.4), 0.7)
    c2w[:3, 3] = (0.3, -0.2, 0.5)
    c2w = c2w.astype(np.float32).astype(np.float64)
    R, t = c2w[:3, :3], c2w[:3, 3]
    pano = ref.rays(views.pano_camera(H, W), c2w)
    theta = -(np.arange(W) + 0.5) * 2 * np.pi / W
    heading = np.stack([np.sin(theta), np.zeros(W), np.cos(theta)], -1)  # the panorama direction at the horizon
    up = np.array([0.0, 1.0, 0.0])
    eyes = {}
    for eye in ("left", "right"):
        r = ref.rays(views.stereo_pano_camera(H, W, ipd, eye), c2w)
        off = ((r["origins"] - t) @ np.linalg.inv(R).T).reshape(H, W, 3)  # camera-space offsets (R is fp32-rounded)
        assert np.abs(np.linalg.norm(off, axis=-1) - np.float32(ipd / 2)).max() <= 1e-15  # on the viewing circle
        assert np.abs((off * heading[None]).sum(-1)).max() <= 1e-15  # tangent: origin perpendicular to the heading
        assert np.abs(off[..., 1]).max() <= 1e-15
        for f in ("directions", "viewdirs", "radii", "noise_var", "lossmult", "near", "far"):
            assert np.array_equal(r[f], pano[f]), f
        eyes[eye] = off
    want = np.cross(heading, up) * np.float64(np.float32(ipd / 2))
    assert np.abs(eyes["right"] - want[None]).max() <= 1e-15
    assert np.abs(eyes["left"] + want[None]).max() <= 1e-15
    # every ray is tangent to the circle: origin . direction = 0 in the horizontal plane
    d = (pano["directions"] @ np.linalg.inv(R).T).reshape(H, W, 3)
    assert np.abs((eyes["right"][..., [0, 2]] * d[..., [0, 2]]).sum(-1)).max() <= 1e-15
    for eye in ("left", "right"):
        zero = ref.rays(views.stereo_pano_camera(H, W, 0.0, eye), c2w)
        for f in pano:
            assert np.array_equal(zero[f], pano[f]), f


# ------------------------------------------------------------------------------------------------------- reprojection
ROT = ref.rotation_matrix((0.3, -0.8, 0.52), 1.234)


def test_constant_image_stays_constant():
    for src in central_cameras():
        for dst in central_cameras():
            img = np.full((2, 3, src.h, src.w), 0.75)
            out, cov = ref.reproject(img, src, dst, ROT, samples=2, fill=-1.0)
            assert out.shape == (2, 3, dst.h, dst.w) and cov.shape == (dst.h, dst.w)
            seen = cov > 0
            assert np.abs(out[:, :, seen] - 0.75).max() <= 1e-12 if seen.any() else True
            assert (out[:, :, ~seen] == -1.0).all()
            assert ((cov >= 0) & (cov <= 1)).all()
            if ref.kind(src) in ("pano", "cube") and ref.kind(dst) != "fisheye":
                assert (cov == 1).all()


@pytest.mark.parametrize("m", [1, 5, -3])
def test_pano_yaw_is_a_column_roll(m):
    H, W = 8, 16
    cam = views.pano_camera(H, W)
    img = np.random.default_rng(3).random((1, 2, H, W))
    a = 2 * np.pi * m / W
    ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    out, cov = ref.reproject(img, cam, cam, ry, round_rotation=False)
    assert (cov == 1).all()
    assert np.abs(out - np.roll(img, m, axis=-1)).max() <= 1e-9
    same, _ = ref.reproject(img, cam, cam)
    assert np.abs(same - img).max() <= 1e-12


def test_pinhole_to_pano_coverage_is_the_frustum():
    src, dst = views.perspective_camera(24, 32, fov_x_deg=90.0), views.pano_camera(32, 64)
    img = np.ones((1, 1, src.h, src.w))
    out, cov = ref.reproject(img, src, dst, fill=7.0)
    d, _ = ref.pix_to_dir(dst, *np.meshgrid(np.arange(dst.w) + 0.5, np.arange(dst.h) + 0.5))
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    inside = (z < 0) & (np.abs(x) < -z * (1 - 1e-6)) & (np.abs(y) < -z * (src.h / src.w) * (1 - 1e-6))
    outside = (z >= 0) | (np.abs(x) > -z * (1 + 1e-6)) | (np.abs(y) > -z * (src.h / src.w) * (1 + 1e-6))
    assert inside.sum() > 100 and (inside | outside).all()
    assert (cov[inside] == 1).all() and (cov[outside] == 0).all()
    assert (cov[z >= 0] == 0).all()  # nothing behind the camera
    assert (out[0, 0][outside] == 7.0).all() and np.abs(out[0, 0][inside] - 1).max() <= 1e-12


# ---------------------------------------------------------------------------------------- orientation, end to end
G_LIN = 0.9 * np.array([0.48, -0.6, 0.64])          # |.| = 0.9: a linear term, brightest towards an oblique direction
LOBE = np.array([0.5, 0.6, -0.62]) / np.linalg.norm([0.5, 0.6, -0.62])  # the bright lobe's axis, off every axis


def radiance(d):
    """smooth HDR radiance, a quadratic polynomial of the direction: 1 + g . d + 2 (c . d)^2"""
    return 1.0 + d @ G_LIN + 2.0 * (d @ LOBE) ** 2


def exact_irradiance(n):
    """integral of radiance(d) max(0, n . d) over the sphere: the bands l = 0, 1, 2 of the polynomial scaled by pi,
    2 pi / 3, pi / 4 (Ramamoorthi & Hanrahan 2001); (c . d)^2 = 1/3 + its traceless part"""
    return math.pi * (1.0 + 2.0 / 3.0) + (2 * math.pi / 3) * (n @ G_LIN) + (math.pi / 4) * 2.0 * ((n @ LOBE) ** 2 - 1.0 / 3.0)


def test_cube_map_orientation_end_to_end():
    H, W, S = 128, 256, 16
    normals = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
                        [0.6, 0.64, -0.48], [-0.36, 0.48, 0.8], [0.28, -0.96, 0.0], [-0.6, -0.48, -0.64]], float)
    assert np.allclose(np.linalg.norm(normals, axis=1), 1)
    exact = np.array([exact_irradiance(n) for n in normals])
    # lighting's panorama quadrature (probe_directions' table) over the panorama of the radiance
    dirs, omega = ref.pano_table(H, W)
    pano = radiance(dirs)
    e_pano = np.array([(pano * np.maximum(0, dirs @ n) * omega).sum() for n in normals])
    # the cube quadrature: texel-centre directions with cube_solid_angles
    cube_cam = views.cubemap_camera(S)
    cd, _ = ref.pix_to_dir(cube_cam, *np.meshgrid(np.arange(S) + 0.5, np.arange(6 * S) + 0.5))
    cd = (cd / np.linalg.norm(cd, axis=-1, keepdims=True)).reshape(-1, 3)
    cw = views.cube_solid_angles(S).reshape(-1)

    def cube_irradiance(cube):
        return np.array([(cube.reshape(-1) * np.maximum(0, cd @ n) * cw).sum() for n in normals])

    gap_pano = np.abs(e_pano - exact).max()
    gap_cube = np.abs(cube_irradiance(radiance(cd)) - exact).max()  # the quadrature's own error, radiance sampled directly
    allowed = 4 * (gap_pano + gap_cube)
    print(f"quadrature gaps to the analytic irradiance: pano {gap_pano:.3e}, cube {gap_cube:.3e}; allowed {allowed:.3e}")
    assert allowed < 0.02 * exact.min()  # the bound itself is tight enough to mean something
    # the cube map as reproject makes it from the panorama
    cube, cov = ref.reproject(pano.reshape(1, 1, H, W), views.pano_camera(H, W), cube_cam)
    assert (cov == 1).all()
    cube = cube[0, 0]
    gap = np.abs(cube_irradiance(cube) - e_pano).max()
    print(f"cube map of the panorama against the panorama quadrature: {gap:.3e}")
    assert gap <= allowed
    # a swapped pair of faces, or a mirrored face, must break it
    faces = cube.reshape(6, S, S)
    swapped = faces[[4, 1, 2, 3, 0, 5]].reshape(6 * S, S)
    assert np.abs(cube_irradiance(swapped) - e_pano).max() > allowed
    mirrored = faces.copy()
    mirrored[2] = mirrored[2][:, ::-1]
    assert np.abs(cube_irradiance(mirrored.reshape(6 * S, S)) - e_pano).max() > allowed


# --------------------------------------------------------------------------------------------------------- validation
def test_constructor_validation():
    for bad in (1, 0, -3, 2.5):
        with pytest.raises(ValueError):
            views.cubemap_camera(bad)
        with pytest.raises(ValueError):
            views.cube_solid_angles(bad)
    assert views.cubemap_camera(2) == views.CubeCamera(12, 2)
    for fov in (0.0, -10.0, 360.5, float("nan")):
        with pytest.raises(ValueError):
            views.fisheye_camera(8, 8, fov_deg=fov)
    with pytest.raises(ValueError):
        views.fisheye_camera(8, 8, focal=0.0)
    with pytest.raises(ValueError):
        views.fisheye_camera(1, 8)
    cam = views.fisheye_camera(6, 10, fov_deg=180.0)
    assert cam.focal == pytest.approx(3.0 / (math.pi / 2)) and cam.fov_deg == 180.0
    for eye in ("middle", "L", None):
        with pytest.raises(ValueError):
            views.stereo_pano_camera(4, 8, 0.06, eye)
    with pytest.raises(ValueError):
        views.stereo_pano_camera(4, 8, -0.01, "left")
    with pytest.raises(ValueError):
        views.stereo_pano_camera(4, 2, 0.06, "left")
    import torch
    img = torch.zeros(3, 4, 8)
    pano, stereo = views.pano_camera(4, 8), views.stereo_pano_camera(4, 8, 0.06, "right")
    for src, dst in ((stereo, pano), (pano, stereo)):
        with pytest.raises(ValueError):
            views.reproject(img, src, dst)
    for k in (0, -1, 1.5, 17):
        with pytest.raises(ValueError):
            views.reproject(img, pano, pano, samples=k)
    with pytest.raises(ValueError):
        views.reproject(img, pano, pano, rotation=np.eye(4))
    with pytest.raises(ValueError):
        views.reproject(torch.zeros(3, 5, 8), pano, pano)  # not the src camera's size
    with pytest.raises(ValueError):
        views.reproject(img, "pano", pano)
    with pytest.raises(RuntimeError):
        views.reproject(img, pano, pano)  # a CPU tensor: there is no host fallback
    with pytest.raises(ValueError):
        views.generate_perspective_rays(views.cubemap_camera(2), np.eye(4))
    with pytest.raises(ValueError):
        views.PerspectiveRayPool(cam, [np.eye(4)])
