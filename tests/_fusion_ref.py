"""numpy fp64 restatement of pn_tsdf_integrate (include/panonerf_hip.h, section "TSDF fusion"), written from the header and
independent of the device code, with the scenes the fusion tests run in.

The scenes live in the analytic room of _relight_ref (a box with a sphere occluder): depth images are the analytic distance
along each pixel's ray (the pinhole's ray not normalised), rounded to fp32, for that module's four cameras at off-grid eyes.

integrate(...) returns fp64 `tsdf` and `weight` (not yet rounded) and a `fragile` mask over voxels: a voxel is fragile if,
for any view that reaches the decision, a discrete decision lies within `tol` (relative) of flipping - floor qx, floor qy,
the cube's face, a validity bound (q_z > 0, the frame's border, theta_max), sdf against -trunc.  (t against depth_max and
the tests of t and w against 0 and inf compare fp32 inputs exactly and cannot flip.)  Both sides compute in fp64 on the same
fp32 inputs; +, -, *, / and sqrt are correctly rounded on both, so only atan2 / hypot may differ, by a few fp64 ulp.
A decision that sits EXACTLY on its boundary because its inputs are exact zeros is not fragile: a panorama's seam
(e_x = 0: theta = 0 or +-pi), its quarter meridians (e_z = 0: theta = +-pi/2), its poles (e_x = e_z = 0: phi = 0 or pi) and
its horizon (e_y = 0: phi = pi/2) give the same exact angles in every libm, and the edge tests rely on them."""
import functools

import numpy as np

import _cameras_ref as cref
import _relight_ref as rr
from pano_nerf_amd import views

F64 = np.float64
TOL = 1e-9


def f32(x):
    return np.asarray(x, np.float32).astype(F64)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def placement(bounds, res):
    """((x0, y0, z0), (dx, dy, dz)) as geometry._placement states it: the step in fp64, both rounded to fp32"""
    lo, hi = [np.asarray(c, F64) for c in bounds]
    step = (hi - lo) / (np.asarray(res, F64) - 1.0)
    return tuple(float(v) for v in f32(lo)), tuple(float(v) for v in f32(step))


def grid(res, lo, step):
    """[nx, ny, nz, 3] fp64 voxel positions: x0 + i dx with every fp32 scalar widened first"""
    ax = [f32(lo[a]) + np.arange(res[a], dtype=F64) * f32(step[a]) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1)


def _near_int(q, tol):
    """q within tol (relative to max(1, |q|)) of an integer"""
    return np.abs(q - np.rint(q)) < tol * np.maximum(1.0, np.abs(q))


def project(cam, e, tol):
    """direction e [.., 3] -> (qx, qy, face, valid, fragile) by the header's inverse projections"""
    k, p = cref.kind(cam), cref._params(cam, F64)
    H, W = cam.h, cam.w
    x, y, z = e[..., 0], e[..., 1], e[..., 2]
    face = np.zeros(x.shape, np.int64)
    valid = np.ones(x.shape, bool)
    frag = np.zeros(x.shape, bool)
    with np.errstate(all="ignore"):
        if k == "pano":
            phi, theta = np.arctan2(np.hypot(x, z), y), np.arctan2(x, z)
            u = -theta / (2.0 * np.pi)
            qx, qy = (u - np.floor(u)) * W, phi / np.pi * H
            frag = (_near_int(qx, tol) & ~((x == 0) | (z == 0))) | (_near_int(qy, tol) & ~((y == 0) | ((x == 0) & (z == 0))))
        elif k == "pinhole":
            m = p["cam2pix"]
            q = [(m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z for r in range(3)]
            front = q[2] > 0
            qz = np.where(front, q[2], 1.0)
            qx, qy = q[0] / qz, q[1] / qz
            valid = front & (qx >= 0) & (qx <= W) & (qy >= 0) & (qy <= H)
            frag = (np.abs(q[2]) < tol * np.sqrt(dot(e, e))) | (front & (_near_int(qx, tol) | _near_int(qy, tol)))
        elif k == "fisheye":
            r = np.hypot(x, y)
            theta = np.arctan2(r, -z)
            inside = theta <= p["tmax"]
            rs = np.where(r > 0, r, 1.0)
            qx = 0.5 * W + np.where(r > 0, (p["f"] * theta) * x / rs, 0.0)
            qy = 0.5 * H - np.where(r > 0, (p["f"] * theta) * y / rs, 0.0)
            valid = inside & (qx >= 0) & (qx <= W) & (qy >= 0) & (qy <= H)
            frag = (np.abs(theta - p["tmax"]) < tol * np.maximum(1.0, theta)) | (inside & (_near_int(qx, tol) | _near_int(qy, tol)))
        else:
            ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
            isx = (ax >= ay) & (ax >= az)
            isy = ~isx & (ay >= az)
            mj = np.where(isx, ax, np.where(isy, ay, az))
            ms = np.where(mj > 0, mj, 1.0)
            face = np.where(isx, np.where(x > 0, 0, 1), np.where(isy, np.where(y > 0, 2, 3), np.where(z > 0, 4, 5)))
            s = np.choose(face, [-z, z, x, x, x, -x]) / ms
            t = np.choose(face, [-y, -y, z, -z, -y, -y]) / ms
            qx, qy = (s + 1.0) * (0.5 * W), (t + 1.0) * (0.5 * W)
            valid = mj > 0
            srt = np.sort(np.stack([ax, ay, az], -1), -1)
            frag = ((srt[..., 2] - srt[..., 1]) < tol * srt[..., 2]) | _near_int(qx, tol) | _near_int(qy, tol)
    return qx, qy, face, valid, frag


def integrate(res, lo, step, cam, c2ws, depth, confidence=None, view_weights=None, trunc=None, depth_max=np.inf,
              max_weight=np.inf, tsdf=None, weight=None, tol=TOL):
    """-> dict tsdf, weight [nx, ny, nz] fp64 (not yet rounded), fragile, seen (bool: some view contributed).
    lo / step are the fp32 values of the grid, depth [S, H, W], c2ws [S, 4, 4]; tsdf / weight: the fp32 volume to continue
    (None: a fresh one)."""
    k = cref.kind(cam)
    H, W = cam.h, cam.w
    rows = W if k == "cube" else H
    depth32 = np.asarray(depth, np.float32).reshape(-1, H, W)
    S = depth32.shape[0]
    conf32 = None if confidence is None else np.asarray(confidence, np.float32).reshape(S, H, W)
    vw32 = None if view_weights is None else np.asarray(view_weights, np.float32).reshape(S)
    trunc = float(f32(trunc))
    dmax32, wmax = np.float32(depth_max), float(f32(max_weight))
    X = grid(res, lo, step)
    A, B = np.zeros(X.shape[:-1]), np.zeros(X.shape[:-1])
    fragile = np.zeros(X.shape[:-1], bool)
    with np.errstate(all="ignore"):
        for s in range(S):
            m = f32(np.asarray(c2ws)[s])
            R, o = m[:3, :3], m[:3, 3]
            v = X - o
            e = np.stack([(R[0, q] * v[..., 0] + R[1, q] * v[..., 1]) + R[2, q] * v[..., 2] for q in range(3)], -1)
            rho = np.sqrt(dot(e, e))
            ok = (rho > 0) & (rho < np.inf)
            es = np.where(ok[..., None], e, np.array([0.3, 0.2, -1.0]))
            qx, qy, face, valid, frag = project(cam, es, tol)
            fragile |= ok & frag
            ok = ok & valid
            col = np.clip(np.floor(np.where(ok, qx, 0.0)), 0, W - 1).astype(np.int64)
            row = np.clip(np.floor(np.where(ok, qy, 0.0)), 0, rows - 1).astype(np.int64) + (face * W if k == "cube" else 0)
            t32 = depth32[s][row, col]
            ok = ok & (t32 > 0) & (t32 < np.inf) & (t32 <= dmax32)
            w = np.full(X.shape[:-1], 1.0 if vw32 is None else float(vw32[s]))
            if conf32 is not None:
                w = w * conf32[s][row, col].astype(F64)
            ok = ok & (w > 0) & (w < np.inf)
            z = t32.astype(F64)
            if k == "pinhole":
                p = cref._params(cam, F64)["pix2cam"]
                px, py = col + 0.5, row + 0.5
                c = np.stack([(p[q, 0] * px + p[q, 1] * py) + p[q, 2] for q in range(3)], -1)
                z = z * np.sqrt(dot(c, c))
            sdf = z - rho
            fragile |= ok & (np.abs(sdf + trunc) < tol * np.maximum(rho, z))
            ok = ok & ~(sdf < -trunc)
            d = np.minimum(1.0, sdf / trunc)
            A = np.where(ok, A + w * d, A)
            B = np.where(ok, B + w, B)
        W0 = np.zeros(A.shape) if weight is None else np.asarray(weight, np.float32).astype(F64)
        D0 = np.zeros(A.shape) if tsdf is None else np.where(W0 == 0, 0.0, np.asarray(tsdf, np.float32).astype(F64))
        seen = B != 0
        W1 = W0 + B
        out_t = np.where(seen, (D0 * W0 + A) / np.where(seen, W1, 1.0), D0 if tsdf is None else np.asarray(tsdf, np.float32).astype(F64))
        out_w = np.where(seen, np.minimum(W1, wmax), W0)
    return dict(tsdf=out_t, weight=out_w, fragile=fragile, seen=seen)


# ------------------------------------------------------------------------------------------------------------ scenes
CAMERAS = rr.VIEWS  # "pano" 16 x 32, "pinhole" 17 x 33, "cube" 8, "fisheye" 16 x 16
EYES = (rr.EYE, np.array([0.93, 0.41, -1.17]), np.array([-1.31, -0.77, 1.23]))  # off every grid below, outside the sphere
ROOM_BOUNDS = ((-2.75, -2.3, -2.75), (2.75, 2.3, 2.75))  # beyond the walls by more than TRUNC: the outer voxels are unseen
GRIDS = {"room": ((5, 6, 7), ROOM_BOUNDS), "cell": ((2, 2, 2), ((-0.42, -0.27, 0.2), (-0.2, -0.02, 0.44)))}
TRUNC = 0.6  # some voxels clamp to 1, some lie in the band, some are behind it
PARITY = [(c, g, s) for c in CAMERAS for g in ("room", "cell") for s in (1, 3)]


def poses(name, n):
    """n poses at EYES: the first as _relight_ref places that camera, the others looking at points of the room (a rotated
    panorama or cube map is as good as an upright one)"""
    targets = (None, np.array([0.2, -0.3, 0.6]), np.array([-0.4, 0.5, -0.2]))
    out = []
    for i in range(n):
        if i == 0:
            m = rr.view_pose(name)
        else:
            m = views.look_at(EYES[i], targets[i], up=(0.1, 1.0, 0.05))
        out.append(m)
    return np.stack(out)


def view_depth(cam, c2w, sphere=True):
    """[H, W] fp32: the analytic distance t of the room along each pixel's ray o + t d, d as the ray generators give it
    (rounded to fp32; the pinhole's not normalised).  Outside a fisheye's circle: the forward ray's, which nothing reads."""
    if cref.kind(cam) == "pinhole":
        m = f32(c2w)
        jj, ii = np.meshgrid(np.arange(cam.w), np.arange(cam.h))
        d = (cref.pix_to_dir(cam, jj + 0.5, ii + 0.5)[0] @ m[:3, :3].T).reshape(-1, 3)
        o = np.broadcast_to(m[:3, 3], d.shape)
    else:
        r = cref.rays(cam, c2w)
        o, d = r["origins"], r["directions"]
    t = rr.intersect(f32(o), f32(d), sphere)[0]
    return t.astype(np.float32).reshape(cam.h, cam.w)


@functools.lru_cache(maxsize=None)
def scene(name, n):
    """(camera, c2ws [n, 4, 4], depth [n, H, W] fp32) of camera `name` at its first n poses"""
    cam = rr.view_camera(name)
    c2ws = poses(name, n)
    return cam, c2ws, np.stack([view_depth(cam, m) for m in c2ws])


def edge_scene(name):
    """The edge inputs of the GPU test, for "pano" or "pinhole": (camera, c2ws [3, 4, 4], depth, confidence, view_weights,
    depth_max, res, bounds).  The first camera sits exactly ON a voxel of a 5 x 6 x 7 grid; the panorama is upright there, so
    its seam, quarter meridians, poles and horizon face grid voxels, and the pinhole leaves voxels behind it.  depth holds
    NaN, 0, negatives, +inf and values above depth_max, confidence zeros and NaN, and the last view's weight is 0."""
    cam = rr.view_camera(name)
    # steps 0.75, 0.4375, 0.625: exact in fp32, and no voxel but those on the camera's axes and planes has an angle that is
    # a rational multiple of pi (no |e_x| = |e_z|, no hypot(e_x, e_z) = |e_y| within the grid)
    res, bounds = (5, 6, 7), ((-1.75, -1.0625, -2.0), (1.25, 1.125, 1.75))
    on_grid = np.array([-0.25, 0.25, 0.5])  # voxel (2, 3, 4)
    c2ws = poses(name, 3)
    c2ws[0, :3, 3] = on_grid
    if name == "pinhole":
        c2ws[0] = views.look_at(on_grid, rr.SPHERE_C + np.array([0.0, 0.1, 0.0]))
    depth = np.stack([view_depth(cam, m) for m in c2ws])
    rng = np.random.default_rng(5)
    bad = np.array([np.nan, 0.0, -1.0, np.inf, -np.inf], np.float32)
    pick = rng.random(depth.shape)
    depth = np.where(pick < 0.3, bad[rng.integers(0, len(bad), depth.shape)], depth).astype(np.float32)
    conf = rng.uniform(0.25, 2.0, depth.shape).astype(np.float32)
    pick = rng.random(depth.shape)
    conf = np.where(pick < 0.15, 0.0, np.where(pick < 0.3, np.nan, conf)).astype(np.float32)
    depth_max = float(np.float32(np.median(depth[np.isfinite(depth) & (depth > 0)]) * 1.5))
    return cam, c2ws, depth, conf, np.array([1.0, 0.5, 0.0], np.float32), depth_max, res, bounds


def sphere_scene(res=24, R=1.0, half=1.3):
    """The geometry test: a constant-depth R panorama 16 x 32 at an off-grid eye, a res^3 grid over eye +- half"""
    eye = np.array([0.137, -0.211, 0.323])
    cam = views.PanoCamera(16, 32)
    c2w = np.eye(4)
    c2w[:3, 3] = eye
    bounds = (tuple(eye - half), tuple(eye + half))
    return cam, c2w[None], np.full((1, 16, 32), R, np.float32), eye, bounds, (res,) * 3
