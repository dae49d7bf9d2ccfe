"""numpy restatement of the camera models of pano_nerf_amd.views and of views.reproject (include/panonerf_hip.h, section
"camera models and reprojection"): every projection, inverse projection, the ray fields and the resampler, written from
the stated conventions and independent of the device code.  Everything runs in the dtype `dt` it is given: float64 is
the reference; float32 is used only to MEASURE how far fp32 arithmetic moves a source coordinate (reference against
reference), from which the GPU tests derive their tolerance."""
import math

import numpy as np

from pano_nerf_amd import views

F64 = np.float64


def kind(cam):
    return {views.PanoCamera: "pano", views.PinholeCamera: "pinhole", views.CubeCamera: "cube",
            views.FisheyeCamera: "fisheye", views.StereoPanoCamera: "stereo"}[type(cam)]


def _params(cam, dt):
    """the camera's numbers as the device receives them: rounded to fp32, then held in dt"""
    k = kind(cam)
    if k == "pinhole":
        m32 = np.asarray(cam.pix2cam, np.float32).reshape(3, 3)
        inv32 = np.linalg.inv(m32.astype(F64)).astype(np.float32)
        return dict(pix2cam=m32.astype(dt), cam2pix=inv32.astype(dt))
    if k == "fisheye":
        return dict(f=dt(np.float32(cam.focal)), tmax=dt(np.float32(math.radians(0.5 * cam.fov_deg))))
    return {}


# ------------------------------------------------------------------------------------------------ pixel -> direction
def cube_table(face, s, t):
    """the cube-map table: camera-space direction of (s, t) on `face` (+x -x +y -y +z -z = 0..5), t pointing down"""
    one = np.ones_like(s)
    table = [(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one)]
    d = np.zeros(np.shape(s) + (3,), np.asarray(s).dtype)
    for f, comps in enumerate(table):
        for k in range(3):
            d[..., k] = np.where(face == f, comps[k], d[..., k])
    return d


def cube_dir(S, px, py, dt=F64):
    px, py = np.asarray(px, dt), np.asarray(py, dt)
    face = np.clip(np.floor(py / dt(S)), 0, 5).astype(np.int64)
    s = dt(2) * px / dt(S) - dt(1)
    t = dt(2) * (py - (face * S).astype(dt)) / dt(S) - dt(1)
    return cube_table(face, s, t), face


def pix_to_dir(cam, px, py, dt=F64):
    """camera-space direction (unit for pano / fisheye, the table's / pix2cam's vector otherwise) of the continuous pixel
    positions (px, py), and the mask of positions the camera covers"""
    k, p = kind(cam), _params(cam, dt)
    px, py = np.asarray(px, dt), np.asarray(py, dt)
    if k in ("pano", "stereo"):
        theta = -(px / dt(cam.w)) * dt(2 * np.pi)
        phi = (py / dt(cam.h)) * dt(np.pi)
        d = np.stack([np.sin(phi) * np.sin(theta), np.cos(phi) + 0 * theta, np.sin(phi) * np.cos(theta)], -1)
        return d.astype(dt), np.ones(px.shape, bool)
    if k == "pinhole":
        v = np.stack([px, py, np.ones_like(px)], -1)
        return (v @ p["pix2cam"].T).astype(dt), np.ones(px.shape, bool)
    if k == "cube":
        return cube_dir(cam.w, px, py, dt)[0], np.ones(px.shape, bool)
    u, v = px - dt(0.5) * dt(cam.w), -(py - dt(0.5) * dt(cam.h))
    r = np.hypot(u, v)
    theta = r / p["f"]
    rs = np.where(r > 0, r, dt(1))
    d = np.stack([np.sin(theta) * u / rs, np.sin(theta) * v / rs, -np.cos(theta)], -1).astype(dt)
    d[r == 0] = (0, 0, -1)
    return d, theta <= p["tmax"]


# ------------------------------------------------------------------------------------------------ direction -> pixel
def dir_to_pix(cam, d, dt=F64):
    """-> dict(px, py: continuous source position (py within the face for a cube), face, valid, margin: distance of the
    sample to the nearest discrete decision (pixels for a frustum border / image circle, relative gap of the two largest
    |components| for a cube; inf where there is none), sin_phi (pano; 1 otherwise))"""
    k, p = kind(cam), _params(cam, dt)
    d = np.asarray(d, dt)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    H, W = cam.h, cam.w
    face = np.zeros(x.shape, np.int64)
    margin = np.full(x.shape, np.inf)
    sin_phi = np.ones(x.shape)
    if k == "pano":
        hyp = np.hypot(x, z)
        phi, theta = np.arctan2(hyp, y), np.arctan2(x, z)
        t = -theta / dt(2 * np.pi)
        t = t - np.floor(t)
        px, py = t * dt(W), phi / dt(np.pi) * dt(H)
        valid = np.ones(x.shape, bool)
        sin_phi = (hyp / np.maximum(np.sqrt(x * x + y * y + z * z), 1e-300)).astype(F64)
    elif k == "pinhole":
        q = d @ p["cam2pix"].T
        qz = np.where(q[..., 2] > 0, q[..., 2], dt(1))
        px, py = q[..., 0] / qz, q[..., 1] / qz
        valid = (q[..., 2] > 0) & (px >= 0) & (px <= W) & (py >= 0) & (py <= H)
        border = np.minimum(np.minimum(np.abs(px), np.abs(px - W)), np.minimum(np.abs(py), np.abs(py - H)))
        margin = np.where(q[..., 2] > 0, border, np.inf).astype(F64)
    elif k == "fisheye":
        rho = np.hypot(x, y)
        theta = np.arctan2(rho, -z)
        r = p["f"] * theta
        rs = np.where(rho > 0, rho, dt(1))
        px = dt(0.5) * dt(W) + np.where(rho > 0, r * x / rs, 0)
        py = dt(0.5) * dt(H) - np.where(rho > 0, r * y / rs, 0)
        valid = (theta <= p["tmax"]) & (px >= 0) & (px <= W) & (py >= 0) & (py <= H)
        border = np.minimum(np.minimum(np.abs(px), np.abs(px - W)), np.minimum(np.abs(py), np.abs(py - H)))
        margin = np.minimum(np.abs(r - p["f"] * p["tmax"]), np.where(theta <= p["tmax"], border, np.inf)).astype(F64)
    else:
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        isx = (ax >= ay) & (ax >= az)
        isy = ~isx & (ay >= az)
        m = np.where(isx, ax, np.where(isy, ay, az))
        ms = np.where(m > 0, m, dt(1))
        face = np.where(isx, np.where(x > 0, 0, 1), np.where(isy, np.where(y > 0, 2, 3), np.where(z > 0, 4, 5)))
        s = np.choose(face, [-z, z, x, x, x, -x]) / ms
        t = np.choose(face, [-y, -y, z, -z, -y, -y]) / ms
        px, py = (s + dt(1)) * (dt(0.5) * dt(W)), (t + dt(1)) * (dt(0.5) * dt(W))
        valid = m > 0
        srt = np.sort(np.stack([ax, ay, az], -1).astype(F64), -1)
        margin = (srt[..., 2] - srt[..., 1]) / np.maximum(srt[..., 2], 1e-300)
    return dict(px=px.astype(dt), py=py.astype(dt), face=face, valid=valid, margin=margin, sin_phi=sin_phi)


# --------------------------------------------------------------------------------------------------------------- rays
def rays(cam, c2w, near=0.0, far=10.0):
    """fp64 ray fields [H W, C] of one camera: the statement of pn_sample_camera_rays (cube, fisheye, stereo) and of the
    panorama camera, on the fp32-rounded c2w."""
    k = kind(cam)
    H, W = cam.h, cam.w
    m = np.asarray(c2w, np.float32).astype(F64)
    R, t = m[:3, :3], m[:3, 3]
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    out = dict(near=np.full((H * W, 1), F64(np.float32(near))), far=np.full((H * W, 1), F64(np.float32(far))))
    if k in ("pano", "stereo"):
        d, _ = pix_to_dir(cam, jj + 0.5, ii + 0.5)
        world = d @ R.T
        out["directions"] = world.reshape(-1, 3)
        out["viewdirs"] = (world / np.linalg.norm(world, axis=-1, keepdims=True)).reshape(-1, 3)
        # constant pixel radius: |dir(H/2, j) - dir(H/2, j + 1)| 2 / sqrt(12); the last column repeats column W - 3
        jc = np.where(jj < W - 1, jj, W - 3)
        a, _ = pix_to_dir(cam, jc + 0.5, np.full(jc.shape, H // 2 + 0.5))
        b, _ = pix_to_dir(cam, jc + 1.5, np.full(jc.shape, H // 2 + 0.5))
        out["radii"] = (np.linalg.norm((a - b) @ R.T, axis=-1) * 2 / math.sqrt(12)).reshape(-1, 1)
        out["noise_var"] = (np.sin((ii + 0.5) / H * np.pi) * np.pi / W).reshape(-1, 1)
        out["lossmult"] = np.ones((H * W, 1))
        org = np.broadcast_to(t, (H, W, 3)).copy()
        if k == "stereo":
            half = F64(np.float32((0.5 if cam.eye == "right" else -0.5) * cam.ipd))
            theta = -(jj + 0.5) * 2 * np.pi / W
            off = half * np.stack([-np.cos(theta), np.zeros_like(theta), np.sin(theta)], -1)
            org = off @ R.T + t
        out["origins"] = org.reshape(-1, 3)
        return out
    rows, top = (W, (ii // W) * W) if k == "cube" else (H, np.zeros_like(ii))

    def unit(i):
        d, inside = pix_to_dir(cam, jj + 0.5, i + 0.5)
        return (d / np.linalg.norm(d, axis=-1, keepdims=True)) @ R.T, inside

    d, inside = unit(ii)
    yy = np.minimum(ii - top, rows - 2)
    a, b = unit(top + yy)[0], unit(top + yy + 1)[0]
    d = np.where(inside[..., None], d, np.array([0.0, 0.0, -1.0]) @ R.T)
    out["directions"] = out["viewdirs"] = d.reshape(-1, 3)
    out["radii"] = (np.linalg.norm(a - b, axis=-1) * 2 / math.sqrt(12)).reshape(-1, 1)
    out["lossmult"] = inside.astype(F64).reshape(-1, 1)
    out["noise_var"] = np.zeros((H * W, 1))
    out["origins"] = np.broadcast_to(t, (H * W, 3)).copy()
    return out


# ------------------------------------------------------------------------------------------------------- reprojection
def sample_coords(src, dst, rotation=None, samples=1, dt=F64, round_rotation=True):
    """every subsample of every destination pixel, [Hd, Wd, k k] in the order b outer, a inner: dir_to_pix's dict of the
    source positions with `valid` also requiring the destination position to be covered.  The rotation is rounded to
    fp32 first, as the device receives it (round_rotation=False keeps it exact, for identities that need it exact)"""
    k = int(samples)
    rot = np.eye(3) if rotation is None else np.asarray(rotation, F64)
    rot = (rot.astype(np.float32) if round_rotation else rot).astype(dt)
    x, y = np.arange(dst.w).astype(dt), np.arange(dst.h).astype(dt)
    sub = (np.arange(k).astype(dt) + dt(0.5)) * (dt(1) / dt(k))
    px = np.broadcast_to((x[None, :, None, None] + sub[None, None, None, :]), (dst.h, dst.w, k, k)).reshape(dst.h, dst.w, k * k)
    py = np.broadcast_to((y[:, None, None, None] + sub[None, None, :, None]), (dst.h, dst.w, k, k)).reshape(dst.h, dst.w, k * k)
    d, ok = pix_to_dir(dst, px, py, dt)
    info = dir_to_pix(src, (d @ rot.T).astype(dt), dt)
    info["valid"] = info["valid"] & ok
    if kind(dst) == "fisheye":  # the destination's own image circle is a decision too
        p = _params(dst, F64)
        r = np.hypot(px.astype(F64) - 0.5 * dst.w, py.astype(F64) - 0.5 * dst.h)
        info["margin"] = np.minimum(info["margin"], np.abs(r - p["f"] * p["tmax"]))
    return info


def fetch(image, src, px, py, face):
    """bilinear fetch of image [N, C, Hs, Ws] (float64) at source positions: taps wrap in a panorama's columns and clamp
    otherwise, a cube's within the face.  -> [N, C, ...]"""
    k = kind(src)
    W = src.w
    rows = W if k == "cube" else src.h
    gx, gy = px - 0.5, py - 0.5
    x0, y0 = np.floor(gx), np.floor(gy)
    wx, wy = gx - x0, gy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    if k == "pano":
        x0, x1 = x0 % W, x1 % W
    else:
        x0, x1 = np.clip(x0, 0, W - 1), np.clip(x1, 0, W - 1)
    top = face * W if k == "cube" else 0
    y0, y1 = top + np.clip(y0, 0, rows - 1), top + np.clip(y1, 0, rows - 1)
    return ((1 - wy) * (1 - wx) * image[:, :, y0, x0] + (1 - wy) * wx * image[:, :, y0, x1]
            + wy * (1 - wx) * image[:, :, y1, x0] + wy * wx * image[:, :, y1, x1])


def reproject(image, src, dst, rotation=None, samples=1, fill=0.0, info=None, round_rotation=True):
    """fp64 statement of views.reproject: -> (out [N, C, Hd, Wd], coverage [Hd, Wd])"""
    img = np.asarray(image, F64)
    if img.ndim == 3:
        img = img[None]
    info = sample_coords(src, dst, rotation, samples, round_rotation=round_rotation) if info is None else info
    v = fetch(img, src, info["px"].astype(F64), info["py"].astype(F64), info["face"])
    ok = info["valid"]
    n = ok.sum(-1)
    total = np.where(ok, v, 0.0).sum(-1)
    out = np.where(n > 0, total / np.maximum(n, 1), fill)
    return out, n / float(ok.shape[-1])


def coord_error(src, dst, rotation, samples):
    """reference against reference: the fp32 restatement's source coordinates against the fp64 one's, per subsample, in
    units of eps scale, eps = 2^-23, scale = Ws / (2 pi sin phi) for a panorama's column and max(Hs, Ws) otherwise.
    -> (ratio_x, ratio_y) over the samples valid in both and away from decisions"""
    eps = float(np.finfo(np.float32).eps)
    a, b = sample_coords(src, dst, rotation, samples, F64), sample_coords(src, dst, rotation, samples, np.float32)
    ok = a["valid"] & b["valid"] & (a["face"] == b["face"]) & (a["margin"] > 1e-4)
    dx = np.abs(a["px"] - b["px"].astype(F64))
    if kind(src) == "pano":
        dx = np.minimum(dx, src.w - dx)
    dy = np.abs(a["py"] - b["py"].astype(F64))
    big = float(max(src.h, src.w))
    sx = src.w / (2 * np.pi * np.maximum(a["sin_phi"], 1e-300)) if kind(src) == "pano" else big
    return (dx / (eps * sx))[ok], (dy / (eps * big))[ok]


# --------------------------------------------------------------------------------------------------- pano quadrature
def pano_table(H, W):
    """(dirs [H W, 3], omega [H W]) of lighting.probe_directions in fp64: pixel-centre directions of the identity panorama
    camera and the midpoint-rule solid angles sin((i + 1/2) pi / H) (2 pi / W) (pi / H)"""
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    d, _ = pix_to_dir(views.PanoCamera(H, W), jj + 0.5, ii + 0.5)
    omega = np.sin((ii + 0.5) / H * np.pi) * (2 * np.pi / W) * (np.pi / H)
    return d.reshape(-1, 3), omega.reshape(-1)


def rotation_matrix(axis, angle):
    a = np.asarray(axis, F64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
