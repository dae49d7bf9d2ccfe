"""Camera models: host-side numpy descriptions of the cameras the ray kernels of ``pn_cameras.hip`` generate rays for.

    perspective_camera(h, w, focal | fov_x_deg | pix2cam)   PinholeCamera(h, w, pix2cam [3, 3] fp32)
    pano_camera(h, w)                           PanoCamera(h, w): the equirectangular camera of generate_pano_rays
    cubemap_camera(size)                        CubeCamera(h = 6 size, w = size): faces +x -x +y -y +z -z as a vertical strip
    fisheye_camera(h, w, fov_deg | focal)       FisheyeCamera(h, w, focal, fov_deg): equidistant, looking along -z
    stereo_pano_camera(h, w, ipd, eye)          StereoPanoCamera(h, w, ipd, eye): one eye of an omnidirectional-stereo pair
    camera_mask(camera)                         bool [H, W]: inside the fisheye's image circle (all true otherwise)
    cube_faces(x)                               [.., C, 6 S, S] -> [.., 6, C, S, S]
    cube_solid_angles(size)                     float64 [6 S, S] exact texel solid angles (sum 4 pi)

A leaf module: ``rays`` (CameraRig) and ``views`` build on it.  Conventions are stated in include/panonerf_hip.h.
"""
import collections
import math

import numpy as np
import torch

PinholeCamera = collections.namedtuple("PinholeCamera", ["h", "w", "pix2cam"])
PanoCamera = collections.namedtuple("PanoCamera", ["h", "w"])
CubeCamera = collections.namedtuple("CubeCamera", ["h", "w"])
FisheyeCamera = collections.namedtuple("FisheyeCamera", ["h", "w", "focal", "fov_deg"])
StereoPanoCamera = collections.namedtuple("StereoPanoCamera", ["h", "w", "ipd", "eye"])
# camera kinds of pn_cameras.hip (include/panonerf_hip.h)
_CAM_PANO, _CAM_PINHOLE, _CAM_CUBE, _CAM_FISHEYE, _CAM_STEREO_PANO = range(5)
_CAM_PARAMS = 20


# ---------------------------------------------------------------------------------------------------------- cameras
def _hw(height, width, min_w=2):
    h, w = int(height), int(width)
    if h < 2 or w < min_w:
        raise ValueError(f"a camera needs height >= 2 and width >= {min_w}; got {height} x {width}")
    return h, w


def perspective_camera(height, width, focal=None, fov_x_deg=None, pix2cam=None):
    """PinholeCamera(h, w, pix2cam [3, 3] fp32).  With a focal length (pixels) or a horizontal field of view (degrees) the
    Blender matrix: pixel (x + 1/2, y + 1/2, 1) -> ((x + 1/2 - w/2) / f, -(y + 1/2 - h/2) / f, -1), x right, y up, looking
    along -z (datasets/base_datasets.py:216-265; focal = w / 2 / tan(fov / 2) as :212-213).  With pix2cam, that matrix as
    given (the Multicam form, :118-170).  h, w >= 2: the cone radius takes the next row's direction."""
    h, w = _hw(height, width)
    if pix2cam is not None:
        if focal is not None or fov_x_deg is not None:
            raise ValueError("give pix2cam, or one of focal and fov_x_deg, not both")
        m = np.asarray(pix2cam, dtype=np.float32)
        if m.shape != (3, 3) or not np.isfinite(m).all():
            raise ValueError(f"pix2cam must be a finite 3x3 matrix; got shape {m.shape}")
        return PinholeCamera(h, w, np.ascontiguousarray(m))
    if (focal is None) == (fov_x_deg is None):
        raise ValueError("give exactly one of focal and fov_x_deg (or pix2cam)")
    if focal is None:
        fov = float(fov_x_deg)
        if not 0.0 < fov < 180.0:
            raise ValueError(f"fov_x_deg must lie in (0, 180); got {fov_x_deg!r}")
        focal = 0.5 * w / math.tan(0.5 * math.radians(fov))
    f = float(focal)
    if not (f > 0.0 and math.isfinite(f)):
        raise ValueError(f"focal must be positive and finite; got {focal!r}")
    m = np.array([[1.0 / f, 0.0, -0.5 * w / f], [0.0, -1.0 / f, 0.5 * h / f], [0.0, 0.0, -1.0]])
    return PinholeCamera(h, w, m.astype(np.float32))


def pano_camera(height, width):
    """PanoCamera(h, w): the equirectangular camera of generate_pano_rays (pn_raygen_pano), for render_view / render_path."""
    return PanoCamera(*_hw(height, width, 3))


def cubemap_camera(size):
    """CubeCamera(h = 6 size, w = size), size >= 2: a cube map as a vertical strip of faces in the order +x, -x, +y, -y,
    +z, -z.  Face texel (x, y) has s = 2 (x + 1/2) / size - 1, t = 2 (y + 1/2) / size - 1 (t points down) and looks along
    +x (1, -t, -s), -x (-1, -t, s), +y (s, 1, t), -y (s, -1, -t), +z (s, -t, 1), -z (-s, -t, -1): the OpenGL cube-map
    table, i.e. the lookup convention of engines (a face viewed as a picture is mirrored relative to a pinhole view)."""
    s = int(size)
    if s != size or s < 2:
        raise ValueError(f"a cube map needs an integer size >= 2; got {size!r}")
    return CubeCamera(6 * s, s)


def fisheye_camera(height, width, fov_deg=180.0, focal=None):
    """FisheyeCamera(h, w, focal, fov_deg): an equidistant fisheye looking along -z like the pinhole, 0 < fov_deg <= 360.
    With u = x + 1/2 - w/2, v = -(y + 1/2 - h/2), r = hypot(u, v), the pixel looks theta = r / focal away from the axis
    along (sin theta u / r, sin theta v / r, -cos theta).  focal (pixels per radian) defaults to (min(h, w) / 2) /
    radians(fov_deg / 2): the image circle touches the shorter side.  A pixel is inside when theta <= radians(fov_deg / 2);
    outside pixels get the forward direction and lossmult = 0, and render_view / render_path return 0 in every channel
    there.  They are still rendered: up to 1 - pi / 4 of the frame's rays for a full circle in a square are spent on
    pixels that end up 0 (there is no compaction of the inside rays)."""
    h, w = _hw(height, width)
    fov = float(fov_deg)
    if not 0.0 < fov <= 360.0:
        raise ValueError(f"fov_deg must lie in (0, 360]; got {fov_deg!r}")
    if focal is None:
        focal = 0.5 * min(h, w) / math.radians(0.5 * fov)
    f = float(focal)
    if not (f > 0.0 and math.isfinite(f)):
        raise ValueError(f"focal must be positive and finite; got {focal!r}")
    return FisheyeCamera(h, w, f, fov)


def stereo_pano_camera(height, width, ipd, eye):
    """StereoPanoCamera(h, w, ipd, eye), eye "left" or "right": one eye of an omnidirectional-stereo (ODS) pair.  Every
    pixel looks along the panorama camera's direction; column j (heading angle theta_j = -(j + 1/2) 2 pi / w) starts at
    the camera-space origin +-(ipd / 2) (-cos theta_j, 0, sin theta_j), + for the right eye: heading x up, so the ray is
    tangent to the viewing circle of diameter ipd.  radii and noise_var are the panorama camera's; with ipd = 0 the rays
    are the panorama camera's bit for bit."""
    h, w = _hw(height, width, 3)
    d = float(ipd)
    if not (d >= 0.0 and math.isfinite(d)):
        raise ValueError(f"ipd must be finite and >= 0; got {ipd!r}")
    if eye not in ("left", "right"):
        raise ValueError(f"eye must be 'left' or 'right'; got {eye!r}")
    return StereoPanoCamera(h, w, d, eye)


def _camera(camera):
    if isinstance(camera, PinholeCamera):
        if np.asarray(camera.pix2cam).shape != (3, 3):
            raise ValueError("PinholeCamera.pix2cam must be 3x3")
        return camera
    if isinstance(camera, CubeCamera):
        if camera.w < 2 or camera.h != 6 * camera.w:
            raise ValueError(f"a CubeCamera is 6 size x size with size >= 2; got {camera.h} x {camera.w}")
        return camera
    if isinstance(camera, FisheyeCamera):
        if not (camera.focal > 0.0 and 0.0 < camera.fov_deg <= 360.0):
            raise ValueError("a FisheyeCamera needs focal > 0 and 0 < fov_deg <= 360")
        return camera
    if isinstance(camera, StereoPanoCamera):
        if camera.eye not in ("left", "right") or not camera.ipd >= 0.0:
            raise ValueError("a StereoPanoCamera needs ipd >= 0 and eye 'left' or 'right'")
        return camera
    if isinstance(camera, PanoCamera):
        return camera
    raise ValueError("camera must come from perspective_camera, pano_camera, cubemap_camera, fisheye_camera or "
                     f"stereo_pano_camera; got {type(camera).__name__}")


def _kind_params(camera):
    """(kind, params float32 [_CAM_PARAMS]) of a camera for pn_cameras.hip (the layout of include/panonerf_hip.h)."""
    p = np.zeros(_CAM_PARAMS, np.float32)
    if isinstance(camera, PinholeCamera):
        m = np.asarray(camera.pix2cam, np.float32).reshape(3, 3)
        p[:9] = m.reshape(9)
        p[9:18] = np.linalg.inv(m.astype(np.float64)).reshape(9)  # cam2pix: inverted in fp64, rounded once
        return _CAM_PINHOLE, p
    if isinstance(camera, CubeCamera):
        return _CAM_CUBE, p
    if isinstance(camera, FisheyeCamera):
        p[0], p[1] = camera.focal, math.radians(0.5 * camera.fov_deg)
        return _CAM_FISHEYE, p
    if isinstance(camera, StereoPanoCamera):
        p[0] = (0.5 if camera.eye == "right" else -0.5) * camera.ipd
        return _CAM_STEREO_PANO, p
    return _CAM_PANO, p


def camera_mask(camera):
    """bool [H, W] numpy: the pixels a camera sees.  For a fisheye, the pixels whose centre lies inside the image circle
    (theta <= radians(fov_deg / 2), evaluated in float64); all true for every other camera."""
    camera = _camera(camera)
    if not isinstance(camera, FisheyeCamera):
        return np.ones((camera.h, camera.w), bool)
    u = np.arange(camera.w) + 0.5 - 0.5 * camera.w
    v = -(np.arange(camera.h) + 0.5 - 0.5 * camera.h)
    return np.hypot(u[None, :], v[:, None]) / camera.focal <= math.radians(0.5 * camera.fov_deg)


def cube_faces(x):
    """[.., C, 6 S, S] -> [.., 6, C, S, S]: the faces (+x, -x, +y, -y, +z, -z) of cube-map strips, as a view where the
    layout allows (torch tensor or numpy array)."""
    shape = tuple(x.shape)
    if len(shape) < 3 or shape[-1] < 1 or shape[-2] != 6 * shape[-1]:
        raise ValueError(f"a cube-map strip is [.., C, 6 S, S]; got {shape}")
    S = shape[-1]
    y = x.reshape(*shape[:-2], 6, S, S)
    return y.movedim(-3, -4) if isinstance(y, torch.Tensor) else np.moveaxis(y, -3, -4)


def cube_solid_angles(size):
    """float64 [6 size, size]: the exact solid angle of every texel of cubemap_camera(size), from the corner function
    A(x, y) = atan2(x y, sqrt(x^2 + y^2 + 1)) of the face plane at distance 1: A(x1, y1) - A(x0, y1) - A(x1, y0) +
    A(x0, y0) over the texel's edges in (s, t).  The sum is 4 pi."""
    S = cubemap_camera(size).w
    e = 2.0 * np.arange(S + 1, dtype=np.float64) / S - 1.0
    x, y = e[None, :], e[:, None]
    a = np.arctan2(x * y, np.sqrt(x * x + y * y + 1.0))
    face = a[1:, 1:] - a[1:, :-1] - a[:-1, 1:] + a[:-1, :-1]
    return np.tile(face, (6, 1))


def _c2w_stack(c2ws, single=False):
    """[n, 4, 4] float64 of one c2w ([4, 4] or [3, 4]) or a sequence of them; ValueError on any other shape."""
    a = np.asarray(c2ws, dtype=np.float64)
    if single:
        a = a[None]
    if a.ndim != 3 or a.shape[0] < 1 or a.shape[1:] not in ((4, 4), (3, 4)):
        raise ValueError("a c2w must be a 4x4 or 3x4 matrix" + ("" if single else " (c2ws: [n, 4, 4] or [n, 3, 4])")
                         + f"; got shape {np.shape(c2ws)}")
    if not np.isfinite(a).all():
        raise ValueError("c2w holds a non-finite value")
    out = np.tile(np.eye(4), (a.shape[0], 1, 1))
    out[:, :3, :] = a[:, :3, :]
    return out
