"""Novel views of a trained model: cameras (pinhole, panorama, cube map, fisheye, stereo panorama), camera paths, viewable
frames, reprojection of images between cameras and depth-aware warping of rendered frames to other poses.

Pano-NeRF's models are trained on panoramas, but what a user renders from a trained model is a new view.  This module
renders one (or a whole path of them) and turns the renderer's outputs into the uint8 images the reference's validation
writes.  Frames run on the HIP device through ``pn_views.hip``, rays (``rays.CameraRig``) and reprojection through
``pn_cameras.hip`` (the renderer's own entry points do the rest), under ``torch.no_grad()`` on the current stream; CPU
tensors raise, there is no host fallback.  Cameras (``cameras.py``, re-exported here) and paths are host-side numpy.

    perspective_camera(h, w, focal | fov_x_deg | pix2cam)   PinholeCamera(h, w, pix2cam [3, 3] fp32)
    pano_camera(h, w)                           PanoCamera(h, w): the equirectangular camera of generate_pano_rays
    cubemap_camera(size)                        CubeCamera(h = 6 size, w = size): faces +x -x +y -y +z -z as a vertical strip
    fisheye_camera(h, w, fov_deg | focal)       FisheyeCamera(h, w, focal, fov_deg): equidistant, looking along -z
    stereo_pano_camera(h, w, ipd, eye)          StereoPanoCamera(h, w, ipd, eye): one eye of an omnidirectional-stereo pair
    camera_mask(camera)                         bool [H, W]: inside the fisheye's image circle (all true otherwise)
    cube_faces(x)                               [.., C, 6 S, S] -> [.., 6, C, S, S]
    cube_solid_angles(size)                     float64 [6 S, S] exact texel solid angles (sum 4 pi)
    generate_camera_rays(camera, c2w, ...)      Rays of [H W, C] device tensors for any camera
    generate_perspective_rays(camera, c2w, ...) Rays of [H W, C] device tensors (datasets/base_datasets.py:118-265)
    PerspectiveRayPool(camera, c2ws, images)    the pinhole counterpart of DeviceRayPool (rays.py): take / sample / rays / len
    interpolate_path(c2ws, n_views)             gen_render_path (utils/vis.py:136-165), numpy only
    spiral_path(radii, focus_depth, n_poses)    create_spiral_poses (utils/vis.py:168-200), as 4x4 matrices
    spheric_path(radius, n_poses)               create_spheric_poses (utils/vis.py:203-242), as 4x4 matrices
    look_at(eye, target, up)                    a c2w whose -z looks from eye at target
    to_frame(image, kind, near, far, exposure)  uint8 [H, W, 3] of one render_image output (utils/vis.py:13-41)
    render_view(model, camera, c2w, ...)        dict of [1, C, H, W] outputs named as render_image's
    render_path(model, camera, poses, ...)      dict kind -> uint8 [n, H, W, 3] frames (or PNG / EXR files)
    render_stereo_pano(model, h, w, ipd, c2w, ...)  render_view's dict, the left eye stacked on the right: [1, C, 2 H, W]
    reproject(image, src_camera, dst_camera, ...)   (out [N, C, Hd, Wd], coverage [Hd, Wd]): resample between cameras
    warp_view(image, depth, src_camera, src_c2w, dst_camera, dst_c2w, ...)   dict image / depth / index / coverage: RGB-D
                                                frames seen from other poses (z-buffered forward splatting)
    render_path_warped(model, camera, poses, key_every, ...)   render_path's frames, every key_every-th pose rendered and
                                                the poses between warped from their two rendered neighbours
                                                (blend=True: blended by weight; inpaint=True: holes filled)
    blend_warps(images, depths, weights, ...)   dict image / depth / coverage: S layers of warped frames blended per pixel
                                                among the layers on the nearest surface
    fill_holes(image, depth, coverage, camera, ...)   dict image / depth / filled: holes filled by a push-pull pyramid that
                                                prefers the background

Conventions (pixel directions, radii, frame bytes, the cube-map table, the inverse projections) are stated in
include/panonerf_hip.h.  The host-side conventions of every path and probe renderer of the package live here too
(DESIGN.md 6r): _FrameSink (frames in memory or as files), _put_groups (whole frames per group of rays), _render_rows (the
one loop from a rig's rows to the field), _probe_rig (identity-rotation cameras at positions), _in_circle (the fisheye
mask) and _image_view (an image argument read through its strides); lighting, relight, emitters, objects and volume
import them.
"""
import math
import os

import numpy as np
import torch

from . import _lib, io_exr
from .geometry import _model_device
from .cameras import (PinholeCamera, PanoCamera, CubeCamera, FisheyeCamera, StereoPanoCamera, perspective_camera,  # noqa
                      pano_camera, cubemap_camera, fisheye_camera, stereo_pano_camera, camera_mask, cube_faces,
                      cube_solid_angles, _camera, _kind_params, _c2w_stack)
from .parallel import lanes
from .rays import Rays, CameraRig, PerspectiveRayPool  # noqa

_MAX_SAMPLES = 16
_MAX_SPLAT = 8  # PN_WARP_MAX_SPLAT
_WARPED_KINDS = ("ldr", "hdr", "depth")

_FRAME_KINDS = {"ldr": 0, "ldr_gt": 1, "depth": 2, "normal": 3, "albedo": 4}
# render_view outputs -> the render_image names they fill
_OUTPUTS = {"rgb": ("coarse_rgb", "fine_rgb"), "depth": ("coarse_dep", "fine_dep"), "normal": ("fine_nor",),
            "albedo": ("albedo",), "surface": ("surface_rgb",), "shading": ("shading",)}
_SURF = ("albedo", "surface", "shading")
# render_path kinds: (render_view output, render_image name, to_frame kind); systems/panonerf_system.py:77-131
_PATH_KINDS = {"ldr": ("rgb", "fine_rgb", "ldr"), "ldr_surf": ("surface", "surface_rgb", "ldr"),
               "depth": ("depth", "fine_dep", "depth"), "normal": ("normal", "fine_nor", "normal"),
               "albedo": ("albedo", "albedo", "albedo"), "hdr": ("rgb", "fine_rgb", None)}
_PATH_GROUP_RAYS = 1 << 22  # rays per group of frames in _put_groups (~220 MB of render_path outputs at most)


def generate_camera_rays(camera, c2w, near=0.0, far=10.0, device="cuda"):
    """One camera of any model -> Rays of [H W, C] fp32 device tensors (row-major pixels): the rays render_view renders
    for it (pn_sample_pano_rays, pn_sample_pinhole_rays or pn_sample_camera_rays over idx = arange(H W))."""
    rig = CameraRig(camera, _c2w_stack(c2w, single=True), device)
    idx = torch.arange(rig.h * rig.w, dtype=torch.int64, device=rig.device)
    return rig.sample(idx, near, far)[0]


def generate_perspective_rays(camera, c2w, near=0.0, far=10.0, device="cuda"):
    """One pinhole camera -> Rays of [H W, C] fp32 device tensors (row-major pixels): pn_sample_pinhole_rays over
    idx = arange(H W), the arithmetic every pinhole ray of this module comes from."""
    if not isinstance(camera, PinholeCamera):
        raise ValueError("camera must come from perspective_camera")
    return generate_camera_rays(camera, c2w, near, far, device)


# ------------------------------------------------------------------------------------------------------------ paths
def _euler_xyz_from_matrix(m):
    """[3] extrinsic x-y-z Euler angles (degrees) of a rotation matrix R = Rz(c) Ry(b) Rx(a), in scipy's ranges
    (a, c in [-180, 180], b in [-90, 90])."""
    a = math.atan2(m[2, 1], m[2, 2])
    b = math.atan2(-m[2, 0], math.hypot(m[0, 0], m[1, 0]))
    c = math.atan2(m[1, 0], m[0, 0])
    return np.degrees(np.array([a, b, c]))


def _matrix_from_euler_xyz(angles):
    a, b, c = np.radians(angles)
    ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, ca, -sa], [0.0, sa, ca]])
    ry = np.array([[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]])
    rz = np.array([[cc, -sc, 0.0], [sc, cc, 0.0], [0.0, 0.0, 1.0]])
    return rz @ ry @ rx


def interpolate_path(c2ws, n_views=30):
    """gen_render_path (utils/vis.py:136-165): [N (n_views // 3), 4, 4] float64 c2ws that run through the N poses and back
    to the first, interpolating Euler 'xyz' angles (extrinsic, degrees) and positions linearly, n_views // 3 per leg.
    As upstream, an angle more than 180 degrees away from the FIRST pose's is unwrapped by +360 (only +360, and only
    relative to the first pose).  Rotations must be proper (orthonormal); pitch near +-90 degrees is gimbal lock."""
    c = _c2w_stack(c2ws)
    k = int(n_views) // 3
    if k < 1:
        raise ValueError(f"n_views must be >= 3; got {n_views!r}")
    weight = np.linspace(1.0, .0, k, endpoint=False).reshape(-1, 1)
    rot, pos, rot_i, pos_i = [], [], [], []
    for i in range(c.shape[0]):
        e = _euler_xyz_from_matrix(c[i, :3, :3]).reshape(1, 3)
        if i:
            mask = np.abs(e - rot[0]) > 180
            e[mask] += 360.0
        rot.append(e)
        pos.append(c[i, :3, 3:].reshape(1, 3))
        if i:
            rot_i.append(weight * rot[i - 1] + (1.0 - weight) * rot[i])
            pos_i.append(weight * pos[i - 1] + (1.0 - weight) * pos[i])
    rot_i.append(weight * rot[-1] + (1.0 - weight) * rot[0])
    pos_i.append(weight * pos[-1] + (1.0 - weight) * pos[0])
    angles, positions = np.concatenate(rot_i), np.concatenate(pos_i)
    out = np.tile(np.eye(4), (angles.shape[0], 1, 1))
    for j in range(angles.shape[0]):
        out[j, :3, :3] = _matrix_from_euler_xyz(angles[j])
        out[j, :3, 3] = positions[j]
    return out


def _normalize(v):
    return v / np.linalg.norm(v)


def _to44(poses):
    p = np.asarray(poses, dtype=np.float64)
    out = np.tile(np.eye(4), (p.shape[0], 1, 1))
    out[:, :3, :] = p
    return out


def spiral_path(radii, focus_depth, n_poses=120):
    """create_spiral_poses (utils/vis.py:168-200) as [n_poses, 4, 4] float64: two turns of a spiral of the given radii
    (3 values) around the origin, every pose looking at (0, 0, -focus_depth)."""
    poses = []
    for t in np.linspace(0, 4 * np.pi, int(n_poses) + 1)[:-1]:
        center = np.array([np.cos(t), -np.sin(t), -np.sin(0.5 * t)]) * radii
        z = _normalize(center - np.array([0, 0, -focus_depth]))
        y_ = np.array([0, 1, 0])
        x = _normalize(np.cross(y_, z))
        y = np.cross(z, x)
        poses += [np.stack([x, y, z, center], 1)]
    return _to44(np.stack(poses, 0))


def spheric_path(radius, n_poses=120):
    """create_spheric_poses (utils/vis.py:203-242) as [n_poses, 4, 4] float64: a circle of poses at distance `radius`,
    looking 36 degrees downwards at the origin."""
    def trans_t(t):
        return np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, t], [0, 0, 0, 1]])

    def rot_phi(phi):
        return np.array([[1, 0, 0, 0], [0, np.cos(phi), -np.sin(phi), 0], [0, np.sin(phi), np.cos(phi), 0], [0, 0, 0, 1]])

    def rot_theta(th):
        return np.array([[np.cos(th), 0, -np.sin(th), 0], [0, 1, 0, 0], [np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1]])

    poses = []
    for th in np.linspace(0, 2 * np.pi, int(n_poses) + 1)[:-1]:
        c2w = rot_theta(th) @ rot_phi(-np.pi / 5) @ trans_t(radius)
        c2w = np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]]) @ c2w
        poses += [c2w[:3]]
    return _to44(np.stack(poses, 0))


def look_at(eye, target, up=(0, 1, 0)):
    """[4, 4] float64 c2w at `eye` whose -z axis points at `target` (the axis construction of create_spiral_poses):
    z = normalize(eye - target), x = normalize(up x z), y = z x x; right-handed, x right, y up, as perspective_camera.

    The same c2w given to an equirectangular camera (pn_raygen_pano, generate_pano_rays) looks along -z at the centre of
    the panorama: the corner shared by pixels (H/2 - 1, W/2 - 1) and (H/2, W/2) (theta = -pi, phi = pi / 2); column
    3 W / 4 looks along +x and row 0 towards +y.  So a perspective view with this c2w shows the middle of the panorama
    rendered at the same pose."""
    e, t, u = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    z = e - t
    if not np.linalg.norm(z) > 0:
        raise ValueError("eye and target coincide")
    z = _normalize(z)
    x = np.cross(u, z)
    if not np.linalg.norm(x) > 1e-12:
        raise ValueError("up is parallel to the viewing direction")
    x = _normalize(x)
    y = np.cross(z, x)
    out = np.eye(4)
    out[:3, :4] = np.stack([x, y, z, e], 1)
    return out


# ----------------------------------------------------------------------------------------------------------- frames
def _jet_lut():
    """matplotlib's 'jet' lookup table ([256, 3], utils/vis.py:13-22 hotmap) from its published segment data, with
    LinearSegmentedColormap's float64 arithmetic, then rounded to float32 as torch.Tensor(h) rounds it."""
    segments = (((0., 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1., 0.5, 0.5)),
                ((0., 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.64, 1, 1), (0.91, 0, 0), (1., 0, 0)),
                ((0., 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1., 0, 0)))
    N = 256
    cols = []
    for data in segments:
        a = np.array(data)
        x, y0, y1 = a[:, 0] * (N - 1), a[:, 1], a[:, 2]
        xind = (N - 1) * np.linspace(0, 1, N) ** 1.0
        ind = np.searchsorted(x, xind)[1:-1]
        distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut = np.concatenate([[y1[0]], distance * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]])
        cols.append(np.clip(lut, 0.0, 1.0))
    return np.stack(cols, 1).astype(np.float32)


JET_LUT = _jet_lut()
_LUTS = {}


def _lut(dev):
    key = str(dev)
    if key not in _LUTS:
        _LUTS[key] = torch.from_numpy(JET_LUT.reshape(-1).copy()).to(dev)
    return _LUTS[key]


def _image_view(image):
    """(x, strides): image ([.., H, W], any dtype) as fp32, read in place where its rows are evenly spaced pixels
    (stride(-2) = W stride(-1): contiguous buffers and the permuted views of [.., H, W, C] buffers alike) and as a
    contiguous copy otherwise.  The kernels take the strides that are left; torch has no negative strides to refuse."""
    x = image.detach()
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if x.stride(-2) != x.shape[-1] * x.stride(-1):
        x = x.contiguous()
    return x, x.stride()


def to_frame(image, kind, near=None, far=None, exposure=0.0):
    """uint8 [H, W, 3] device tensor: the bytes the reference's validation writes for one [1, C, H, W] render_image
    output (systems/panonerf_system.py:77-131 through save_results, utils/vis.py:25-41), read in place through its strides.

        "ldr"     hdr_to_ldr(x, dtype='uint8')   (pred_ldr, pred_ldr_surf)
        "ldr_gt"  hdr_to_ldr(x)                  (gt_ldr: no quantisation)
        "depth"   hotmap((d - near) / (far - near)), min / max over the image (C = 1; needs near and far)
        "normal"  (F.normalize(n, dim=1) + 1) / 2
        "albedo"  albedo, clamped to [0, 1]

    exposure scales the HDR input of "ldr" / "ldr_gt" by 2 ** exposure first (0: the reference's bytes).  A NaN depth
    anywhere gives a black frame, as upstream's hotmap does."""
    if kind not in _FRAME_KINDS:
        raise ValueError(f"kind must be one of {sorted(_FRAME_KINDS)}; got {kind!r}")
    if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[0] != 1:
        raise ValueError(f"image must be a [1, C, H, W] tensor; got {getattr(image, 'shape', type(image))}")
    C, H, W = (int(s) for s in image.shape[1:])
    want = 1 if kind == "depth" else 3
    if C != want:
        raise ValueError(f"a {kind!r} frame takes {want} channel(s); got {C}")
    if H < 1 or W < 1:
        raise ValueError("image is empty")
    if image.device.type != "cuda":
        raise RuntimeError("pano_nerf_amd.views runs on a HIP device only (the image is on %s); there is no CPU fallback"
                           % image.device)
    near_f, range_f = 0.0, 1.0
    if kind == "depth":
        if near is None or far is None:
            raise ValueError("a depth frame needs near and far")
        near_f, range_f = float(near), float(far - near)  # far - near in double, rounded once (as Python does upstream)
    dev = image.device
    x, (cs, _, sw) = _image_view(image[0])
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        work = torch.empty(2, dtype=torch.float32, device=dev) if kind == "depth" else None
        _lib.call("pn_to_frame", _FRAME_KINDS[kind], H, W, x.data_ptr(), cs, sw, float(2.0 ** float(exposure)), near_f,
                  range_f, _lib.ptr(_lut(dev) if kind == "depth" else None), _lib.ptr(work), out.data_ptr(), _lib.stream(dev))
    return out


# -------------------------------------------------------------------------------------------------------- rendering
def _flags(model, outputs, env_rays):
    """-> (surf, normals) of the least renderer configuration that yields `outputs`."""
    outputs = tuple(outputs)
    bad = [o for o in outputs if o not in _OUTPUTS]
    if bad or not outputs:
        raise ValueError(f"outputs must be a non-empty subset of {sorted(_OUTPUTS)}; got {outputs!r}")
    surf = any(o in _SURF for o in outputs)
    if surf:
        if model._NC != 5:
            raise ValueError(f"{type(model).__name__} has no surface outputs ({', '.join(_SURF)}): use a PanoMipNeRF")
        if env_rays is None:
            raise ValueError("surface outputs need env_rays (e.g. generate_lit_rays(10, radius))")
    return surf, surf or "normal" in outputs


def _in_circle(camera, rays, rows):
    """rows (name -> [n, C]) with 0 in every channel outside a fisheye's image circle; any other camera's as they are"""
    if not isinstance(camera, FisheyeCamera):
        return rows
    seen = rays.lossmult > 0
    return {k: torch.where(seen, v, 0.0) for k, v in rows.items()}


def _render_rows(model, rig, first, count, env_rays, surf, normals, near, far, chunk, bufs, streams=2):
    """Render rays [first, first + count) of the (frame, pixel) index space into bufs[name][0:count]: the one loop that
    feeds a rig's rows to the field for inference.  The chunks are dealt to `streams` HIP streams with the weight packs
    built once and frozen, as render_image deals them (the same kernels on the same rays: the same bits); with
    streams=1 everything runs on the current stream and nothing is packed ahead or frozen (the probes)."""
    dev = rig.device
    starts = list(range(0, count, chunk))
    # (with surface outputs the cached fp32 env rays are made on this stream, before the other lanes fork from it)
    with lanes(model, dev, min(int(streams), len(starts)), env_rays if surf else None) as lane:
        for i, s in enumerate(starts):
            with torch.cuda.stream(lane[i % len(lane)]):
                n = min(chunk, count - s)
                idx = torch.arange(first + s, first + s + n, dtype=torch.int64, device=dev)
                rays, _ = rig.sample(idx, near, far)
                outs, _ = model._run(rays, env_rays if surf else None, False, False, surf, False, normals)
                comp0, dist0, comp1, dist1, _, normal, albedo, surface, _, shading = outs
                got = dict(coarse_rgb=comp0, fine_rgb=comp1, coarse_dep=dist0, fine_dep=dist1, fine_nor=normal,
                           albedo=albedo, surface_rgb=surface, shading=shading)
                rows = _in_circle(rig.camera, rays, {name: got[name].reshape(n, -1) for name in bufs})
                for name, buf in bufs.items():
                    buf[s:s + n].copy_(rows[name])


def _chunk_rays(chunk_rays):
    chunk = int(chunk_rays)
    if chunk <= 0:
        raise ValueError(f"chunk_rays must be positive; got {chunk_rays!r}")
    return chunk


def _setup(model, camera, chunk_rays):
    camera = _camera(camera)
    dev = _model_device(model)
    if dev.type != "cuda":
        raise RuntimeError("pano_nerf_amd.views renders on a HIP device only (the model is on %s); there is no CPU "
                           "fallback" % dev)
    return camera, dev, _chunk_rays(chunk_rays)


def _probe_positions(positions):
    """P of a [P, 3] positions tensor"""
    if not isinstance(positions, torch.Tensor) or positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError(f"positions must be a [P, 3] tensor; got {getattr(positions, 'shape', type(positions))}")
    return int(positions.shape[0])


def _probe_rig(positions, camera, dev):
    """The CameraRig of P identity-rotation cameras at positions ([P, 3] tensor on dev): what every probe, shadow map and
    volume probe is seen from, so that their pixel (p, i, j) looks along the same ray."""
    P = int(positions.shape[0])
    c2ws = torch.eye(4, dtype=torch.float32, device=dev).repeat(P, 1, 1)
    c2ws[:, :3, 3] = positions.detach().to(torch.float32)
    return CameraRig(camera, c2ws, dev)


_WIDTH = dict(coarse_rgb=3, fine_rgb=3, coarse_dep=1, fine_dep=1, fine_nor=3, albedo=3, surface_rgb=3, shading=3)


class _FrameSink:
    """Where a path renderer's frames go: `frames`, kind -> [n, H, W, 3] tensors on `dev` (uint8; fp32 for "hdr"), or with
    out_dir the files out_dir/<kind>/<i:05d>.png (hdr/<i:05d>.exr), written as the frames arrive, and `frames` stays {}."""

    def __init__(self, kinds, n, h, w, dev, out_dir=None):
        self.kinds, self.n, self.h, self.w, self.out_dir, self.frames = tuple(kinds), n, h, w, out_dir, {}
        for k in self.kinds:
            if out_dir is None:
                self.frames[k] = torch.empty(n, h, w, 3, dtype=torch.float32 if k == "hdr" else torch.uint8, device=dev)
            else:
                os.makedirs(os.path.join(out_dir, k), exist_ok=True)

    def put(self, kind, i, frame):
        """frame [H, W, 3] (any strides) is frame i of `kind`"""
        if self.out_dir is None:
            self.frames[kind][i].copy_(frame)
            return
        pixels = frame.contiguous().cpu().numpy()
        if kind == "hdr":
            io_exr.write_exr(os.path.join(self.out_dir, kind, f"{i:05d}.exr"), pixels)
        else:
            io_exr.write_png(os.path.join(self.out_dir, kind, f"{i:05d}.png"), pixels)


def _put_groups(sink, rows, table, near, far, exposure):
    """Fill `sink` from rows over the (frame, pixel) index space, a group of whole frames (at most _PATH_GROUP_RAYS rays)
    at a time: rows(first_ray, count) -> name -> [count, C] fp32; table: kind -> (row name, to_frame kind, or None for
    the rows themselves).  exposure applies to "ldr" frames only."""
    HW = sink.h * sink.w
    group = max(1, min(sink.n, _PATH_GROUP_RAYS // HW))
    for g0 in range(0, sink.n, group):
        nf = min(group, sink.n - g0)
        got = rows(g0 * HW, nf * HW)
        for f in range(nf):
            for k in sink.kinds:
                name, kind = table[k]
                frame = got[name][f * HW:(f + 1) * HW].view(sink.h, sink.w, -1)
                if kind is not None:
                    frame = to_frame(frame[None].permute(0, 3, 1, 2), kind, near, far, exposure if kind == "ldr" else 0.0)
                sink.put(k, g0 + f, frame)


def render_view(model, camera, c2w, env_rays=None, outputs=("rgb", "depth", "normal"), near=0.0, far=10.0,
                chunk_rays=32768):
    """One view -> dict of [1, C, H, W] fp32 tensors named as render_image's (coarse_rgb, fine_rgb for "rgb"; coarse_dep,
    fine_dep for "depth"; fine_nor for "normal"; albedo, surface_rgb, shading).  camera: perspective_camera(...),
    pano_camera(h, w), cubemap_camera(size) (a 6 size x size strip), fisheye_camera(...) (0 outside the image circle) or
    stereo_pano_camera(...).  Runs the least renderer configuration the outputs need: rgb and depth take the two levels only,
    "normal" adds the density-gradient sweep, albedo / surface / shading add the light gather (a PanoMipNeRF and env_rays
    required).  PanoMipNeRF and MipNeRF both work."""
    camera, dev, chunk = _setup(model, camera, chunk_rays)
    surf, normals = _flags(model, outputs, env_rays)
    c2ws = _c2w_stack(c2w, single=True)
    H, W = camera.h, camera.w
    names = [k for o in outputs for k in _OUTPUTS[o]]
    bufs = {k: torch.empty(H * W, _WIDTH[k], dtype=torch.float32, device=dev) for k in dict.fromkeys(names)}
    with torch.no_grad(), torch.cuda.device(dev):
        rig = CameraRig(camera, c2ws, dev)
        _render_rows(model, rig, 0, H * W, env_rays, surf, normals, near, far, chunk, bufs)
    return {k: v.view(1, H, W, -1).permute(0, 3, 1, 2) for k, v in bufs.items()}


def render_path(model, camera, poses, env_rays=None, kinds=("ldr", "depth", "normal"), near=0.0, far=10.0, exposure=0.0,
                out_dir=None, chunk_rays=32768):
    """Render every pose of poses ([n, 4, 4] or [n, 3, 4] c2ws) and turn the outputs into frames: dict kind -> uint8
    [n, H, W, 3] device tensor, each frame to_frame of the render_view output the reference's validation takes for it
    (ldr <- fine_rgb, ldr_surf <- surface_rgb, depth <- fine_dep with near / far, normal <- fine_nor, albedo <- albedo);
    "hdr" is fine_rgb itself as fp32 [n, H, W, 3].  Rays are indexed over (frame, pixel), so small frames share full
    chunks.  With out_dir, frames go to out_dir/<kind>/<i:05d>.png (hdr/<i:05d>.exr) as they complete and the returned
    dict is empty."""
    camera, dev, chunk = _setup(model, camera, chunk_rays)
    kinds = tuple(kinds)
    bad = [k for k in kinds if k not in _PATH_KINDS]
    if bad or not kinds:
        raise ValueError(f"kinds must be a non-empty subset of {sorted(_PATH_KINDS)}; got {kinds!r}")
    outputs = tuple(dict.fromkeys(_PATH_KINDS[k][0] for k in kinds))
    surf, normals = _flags(model, outputs, env_rays)
    c2ws = _c2w_stack(poses)
    names = tuple(dict.fromkeys(_PATH_KINDS[k][1] for k in kinds))
    sink = _FrameSink(kinds, c2ws.shape[0], camera.h, camera.w, dev, out_dir)

    def rows(first, count):
        bufs = {k: torch.empty(count, _WIDTH[k], dtype=torch.float32, device=dev) for k in names}
        _render_rows(model, rig, first, count, env_rays, surf, normals, near, far, chunk, bufs)
        return bufs

    with torch.no_grad(), torch.cuda.device(dev):
        rig = CameraRig(camera, c2ws, dev)
        _put_groups(sink, rows, {k: _PATH_KINDS[k][1:] for k in kinds}, near, far, exposure)
    return sink.frames


def render_stereo_pano(model, height, width, ipd, c2w, env_rays=None, outputs=("rgb", "depth", "normal"), near=0.0,
                       far=10.0, chunk_rays=32768):
    """An omnidirectional-stereo pair -> render_view's dict with the left eye stacked on top of the right: [1, C, 2 H, W]
    (the top-bottom layout headsets take).  Exactly render_view of stereo_pano_camera(height, width, ipd, "left") and
    (..., "right"), concatenated along the rows."""
    eyes = [render_view(model, stereo_pano_camera(height, width, ipd, eye), c2w, env_rays, outputs, near, far, chunk_rays)
            for eye in ("left", "right")]
    return {k: torch.cat([eyes[0][k], eyes[1][k]], 2) for k in eyes[0]}


# ----------------------------------------------------------------------------------------------------- reprojection
def reproject(image, src_camera, dst_camera, rotation=None, samples=1, fill=0.0):
    """Resample image ([C, Hs, Ws] or [N, C, Hs, Ws] fp32 device tensor, any C, seen by src_camera) into dst_camera's
    pixels: -> (out [N, C, Hd, Wd] fp32, coverage [Hd, Wd] fp32), one fused kernel (pn_reproject).  Either camera may be
    a panorama, pinhole, cube-map or fisheye camera; a stereo-panorama camera is not a central projection and raises
    ValueError.  rotation: 3x3 matrix taking a dst camera-space direction to a src camera-space direction (identity by
    default); for two posed cameras at one position it is R_src_c2w^T R_dst_c2w.

    Every destination pixel takes samples x samples positions (x + (a + 1/2) / samples, y + (b + 1/2) / samples), sends
    each through the dst camera to a direction, rotates it, projects it with the src camera and fetches bilinearly (a
    panorama wraps in columns; everything else clamps; a cube clamps within the face).  out is the mean of the valid
    subsamples (fp32, fixed order), coverage their fraction; with none, every channel is `fill`.  NaN in the source
    propagates.  Repeated calls give the same bits.  Permuted views (e.g. [N, H, W, C] buffers) are read in place."""
    src, dst = _camera(src_camera), _camera(dst_camera)
    if isinstance(src, StereoPanoCamera) or isinstance(dst, StereoPanoCamera):
        raise ValueError("a stereo-panorama camera is not a central projection: it cannot be reprojected")
    k = int(samples)
    if k != samples or not 1 <= k <= _MAX_SAMPLES:
        raise ValueError(f"samples must be an integer in [1, {_MAX_SAMPLES}]; got {samples!r}")
    rot = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64)
    if rot.shape != (3, 3) or not np.isfinite(rot).all():
        raise ValueError(f"rotation must be a finite 3x3 matrix; got shape {rot.shape}")
    if not isinstance(image, torch.Tensor) or image.dim() not in (3, 4):
        raise ValueError(f"image must be a [C, Hs, Ws] or [N, C, Hs, Ws] tensor; got {getattr(image, 'shape', type(image))}")
    x = image.detach()
    if x.dim() == 3:
        x = x[None]
    N, C, Hs, Ws = (int(v) for v in x.shape)
    if N < 1 or C < 1:
        raise ValueError("image is empty")
    if (Hs, Ws) != (src.h, src.w):
        raise ValueError(f"image is {Hs} x {Ws} but src_camera is {src.h} x {src.w}")
    if x.device.type != "cuda":
        raise RuntimeError("pano_nerf_amd.views runs on a HIP device only (the image is on %s); there is no CPU fallback"
                           % x.device)
    x, (sn, sc, _, sw) = _image_view(x)
    dev = x.device
    (sk, sp), (dk, dp) = _kind_params(src), _kind_params(dst)
    r32 = np.ascontiguousarray(rot.astype(np.float32).reshape(9))
    out = torch.empty(N, C, dst.h, dst.w, dtype=torch.float32, device=dev)
    cov = torch.empty(dst.h, dst.w, dtype=torch.float32, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        _lib.call("pn_reproject", N, C, sk, src.h, src.w, sp.ctypes.data, dk, dst.h, dst.w, dp.ctypes.data, r32.ctypes.data,
                  k, float(fill), x.data_ptr(), sn, sc, sw, out.data_ptr(), cov.data_ptr(), _lib.stream(dev))
    return out, cov


# ---------------------------------------------------------------------------------------------------------- warping
def _poses(c2w, what):
    """[n, 4, 4] float64 of one pose ([4, 4] or [3, 4]) or a stack of them (array, sequence or tensor)"""
    if isinstance(c2w, torch.Tensor):
        c2w = c2w.detach().cpu().numpy()
    a = np.asarray(c2w, dtype=np.float64)
    try:
        return _c2w_stack(a, single=a.ndim == 2)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None


def warp_view(image, depth, src_camera, src_c2w, dst_camera, dst_c2w, max_splat=4, splat_scale=1.0, fill=0.0):
    """See S RGB-D frames of src_camera at the poses src_c2w from D other poses dst_c2w of dst_camera: every source pixel
    is lifted to its world point, projected into each destination and splatted over its footprint there, a z-buffer
    keeping the nearest point per destination pixel (pn_warp_splat, pn_warp_resolve; the formulas are in
    include/panonerf_hip.h).  Six degrees of freedom at the cost of two small kernels, where render_view costs a full
    render; what no source saw stays a hole.

    image: [S, C, Hs, Ws] or [C, Hs, Ws] device tensor (any C; permuted views are read in place), or None.  depth:
    [S, 1, Hs, Ws], [S, Hs, Ws] or [Hs, Ws], the distance t along the ray CameraRig.sample gives each pixel, i.e.
    render_view's fine_dep as it is (for a pinhole that ray is not normalised, so t is not the Euclidean distance);
    NaN, Inf, 0 and negative depths are no points.  src_c2w / dst_c2w: [S, 4, 4] / [D, 4, 4] (or [., 3, 4], or one pose).
    Cameras: panorama, pinhole, cube map or fisheye on either side; a stereo-panorama camera raises ValueError.

    -> dict: "image" [D, C, Hd, Wd] (absent when image is None; `fill` in holes), "depth" [D, 1, Hd, Wd] (t along the
    destination camera's rays; NaN in holes), "index" [D, Hd, Wd] int64 (the source pixel s Hs Ws + i Ws + j each pixel
    shows; -1 in holes), "coverage" [D, Hd, Wd] (1 where a point landed, 0 in holes).

    A point covers k x k destination pixels, k = min(max_splat, max(1, ceil(splat_scale * its source pixel's angular size
    seen from the destination, in destination pixels))): moving closer magnifies a surface, and with k = 1 the background
    would show between its points.  max_splat in [1, 8].  The result does not depend on the order the points arrive in:
    repeated calls give the same bits.  So render_view's dict plugs in: warp_view(out["fine_rgb"], out["fine_dep"], ...)."""
    src, dst = _camera(src_camera), _camera(dst_camera)
    if isinstance(src, StereoPanoCamera) or isinstance(dst, StereoPanoCamera):
        raise ValueError("a stereo-panorama camera is not a central projection: it cannot be warped")
    k = int(max_splat)
    if k != max_splat or not 1 <= k <= _MAX_SPLAT:
        raise ValueError(f"max_splat must be an integer in [1, {_MAX_SPLAT}]; got {max_splat!r}")
    scale = float(splat_scale)
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError(f"splat_scale must be positive and finite; got {splat_scale!r}")
    if not isinstance(depth, torch.Tensor) or depth.dim() not in (2, 3, 4) or (depth.dim() == 4 and depth.shape[1] != 1):
        raise ValueError("depth must be a [S, 1, Hs, Ws], [S, Hs, Ws] or [Hs, Ws] tensor; got "
                         f"{getattr(depth, 'shape', type(depth))}")
    Hs, Ws = (int(v) for v in depth.shape[-2:])
    if (Hs, Ws) != (src.h, src.w):
        raise ValueError(f"depth is {Hs} x {Ws} but src_camera is {src.h} x {src.w}")
    z = depth.detach().reshape(-1, Hs, Ws)
    S = int(z.shape[0])
    if S < 1:
        raise ValueError("depth is empty")
    x = None
    if image is not None:
        if not isinstance(image, torch.Tensor) or image.dim() not in (3, 4):
            raise ValueError("image must be a [C, Hs, Ws] or [S, C, Hs, Ws] tensor or None; got "
                             f"{getattr(image, 'shape', type(image))}")
        x = image.detach()
        if x.dim() == 3:
            x = x[None]
        if x.shape[1] < 1:
            raise ValueError("image is empty")
        if tuple(x.shape[2:]) != (Hs, Ws):
            raise ValueError(f"image is {x.shape[2]} x {x.shape[3]} but src_camera is {src.h} x {src.w}")
        if x.shape[0] != S:
            raise ValueError(f"image holds {x.shape[0]} frames but depth {S}")
    sc2w, dc2w = _poses(src_c2w, "src_c2w"), _poses(dst_c2w, "dst_c2w")
    if sc2w.shape[0] != S:
        raise ValueError(f"src_c2w holds {sc2w.shape[0]} poses but depth {S} frames")
    D = int(dc2w.shape[0])
    if S * Hs * Ws >= 1 << 32 or D * dst.h * dst.w >= 1 << 31:
        raise ValueError("too many pixels: S Hs Ws must be below 2^32 and D Hd Wd below 2^31")
    for t, what in ((z, "depth"), (x, "image")):
        if t is not None and t.device.type != "cuda":
            raise RuntimeError("pano_nerf_amd.views runs on a HIP device only (the %s is on %s); there is no CPU fallback"
                               % (what, t.device))
    dev = z.device
    if x is not None and x.device != dev:
        raise ValueError(f"image is on {x.device} but depth on {dev}")
    z = z.to(torch.float32).contiguous()
    C, sn, sc, sw = 0, 0, 0, 0
    if x is not None:
        x, (sn, sc, _, sw) = _image_view(x)
        C = int(x.shape[1])
    (sk, sp), (dk, dp) = _kind_params(src), _kind_params(dst)
    Hd, Wd = dst.h, dst.w
    with torch.no_grad(), torch.cuda.device(dev):
        mats = np.concatenate([sc2w, dc2w]).astype(np.float32).reshape(S + D, 16)
        mats = torch.from_numpy(mats).to(dev)  # one upload for both sets of poses
        ms, md = mats[:S], mats[S:]
        zbuf = torch.full((D, Hd, Wd), -1, dtype=torch.int64, device=dev)  # all ones: PN_WARP_EMPTY
        out = torch.empty(D, C, Hd, Wd, dtype=torch.float32, device=dev) if x is not None else None
        dep = torch.empty(D, 1, Hd, Wd, dtype=torch.float32, device=dev)
        index = torch.empty(D, Hd, Wd, dtype=torch.int64, device=dev)
        cov = torch.empty(D, Hd, Wd, dtype=torch.float32, device=dev)
        st = _lib.stream(dev)
        _lib.call("pn_warp_splat", S, sk, Hs, Ws, sp.ctypes.data, z.data_ptr(), ms.data_ptr(), D, dk, Hd, Wd, dp.ctypes.data,
                  md.data_ptr(), k, scale, zbuf.data_ptr(), st)
        _lib.call("pn_warp_resolve", S, C, Hs, Ws, D, dk, Hd, Wd, dp.ctypes.data, zbuf.data_ptr(), _lib.ptr(x), sn, sc, sw,
                  float(fill), _lib.ptr(out), dep.data_ptr(), index.data_ptr(), cov.data_ptr(), st)
    res = {"depth": dep, "index": index, "coverage": cov}
    if out is not None:
        res["image"] = out
    return res


def _depth_ratio(depth_ratio):
    r = float(depth_ratio)
    if not 0.0 <= r < 1.0:  # NaN fails too
        raise ValueError(f"depth_ratio must lie in [0, 1); got {depth_ratio!r}")
    return r


def _on_device(t, what):
    if t.device.type != "cuda":
        raise RuntimeError("pano_nerf_amd.views runs on a HIP device only (the %s is on %s); there is no CPU fallback"
                           % (what, t.device))


def blend_warps(images, depths, weights, depth_ratio=0.05, fill=0.0):
    """Blend S layers of D warped frames by weight, per pixel, among the layers that show the nearest surface (pn_warp_blend;
    the rule is in include/panonerf_hip.h).  images: [S, D, C, H, W] device tensor, e.g. torch.stack of the "image" of S
    single-source warp_view calls; depths: [S, D, H, W] or [S, D, 1, H, W], their "depth"; weights: [S, D] or [S] (one
    weight per layer for every frame), positive and finite.

    A layer counts at a pixel iff 0 < z < inf.  With zn the smallest such z, the layers with z (1 - depth_ratio) <= zn are
    kept and the others are occluded; one kept layer is copied bit for bit, several give (sum w v) / (sum w) in layer
    order, for the colours and the depth.  depth_ratio = 0.05 is a convention, not a measurement.
    -> dict "image" [D, C, H, W], "depth" [D, 1, H, W], "coverage" [D, H, W] (warp_view's shapes): where no layer counts,
    `fill`, NaN and 0; coverage 1 elsewhere."""
    r = _depth_ratio(depth_ratio)
    if not isinstance(images, torch.Tensor) or images.dim() != 5:
        raise ValueError(f"images must be a [S, D, C, H, W] tensor; got {getattr(images, 'shape', type(images))}")
    S, D, C, H, W = (int(v) for v in images.shape)
    if min(S, D, C, H, W) < 1:
        raise ValueError("images is empty")
    if not isinstance(depths, torch.Tensor) or tuple(depths.shape) not in ((S, D, H, W), (S, D, 1, H, W)):
        raise ValueError(f"depths must be [S, D, H, W] = {(S, D, H, W)} (or [S, D, 1, H, W]); got "
                         f"{getattr(depths, 'shape', type(depths))}")
    if S * D * C * H * W >= 1 << 31:
        raise ValueError("too many values: S D C H W must be below 2^31")
    if isinstance(weights, torch.Tensor):
        weights = weights.detach().cpu().numpy()
    w = np.asarray(weights, dtype=np.float64)
    if w.shape == (S,):
        w = np.repeat(w[:, None], D, 1)
    if w.shape != (S, D):
        raise ValueError(f"weights must be [S, D] = {(S, D)} or [S]; got shape {w.shape}")
    w32 = np.ascontiguousarray(w.astype(np.float32))
    if not (np.isfinite(w32).all() and (w32 > 0).all()):
        raise ValueError("weights must be positive and finite")
    _on_device(images, "images")
    _on_device(depths, "depths")
    dev = images.device
    if depths.device != dev:
        raise ValueError(f"depths is on {depths.device} but images on {dev}")
    x = images.detach().to(torch.float32).contiguous()
    z = depths.detach().to(torch.float32).contiguous()
    with torch.no_grad(), torch.cuda.device(dev):
        wd = torch.from_numpy(w32).to(dev)
        out = torch.empty(D, C, H, W, dtype=torch.float32, device=dev)
        dep = torch.empty(D, 1, H, W, dtype=torch.float32, device=dev)
        cov = torch.empty(D, H, W, dtype=torch.float32, device=dev)
        _lib.call("pn_warp_blend", S, D, C, H, W, x.data_ptr(), z.data_ptr(), wd.data_ptr(), r, float(fill), out.data_ptr(),
                  dep.data_ptr(), cov.data_ptr(), _lib.stream(dev))
    return {"image": out, "depth": dep, "coverage": cov}


_FILL_ALL_LEVELS = 32  # PN_FILL_ALL_LEVELS
_DOMAINS = {}


def _domain(camera, dev):
    """uint8 [H, W] device tensor of camera_mask(camera), made once per camera and device"""
    key = (camera, str(dev))
    if key not in _DOMAINS:
        _DOMAINS[key] = torch.from_numpy(np.ascontiguousarray(camera_mask(camera), dtype=np.uint8)).to(dev)
    return _DOMAINS[key]


def fill_holes(image, depth=None, coverage=None, camera=None, depth_ratio=0.05, levels=None):
    """Fill the holes of N frames by push-pull over an image pyramid that prefers the background (pn_fill_holes; the rule
    is in include/panonerf_hip.h): a disocclusion shows what lay BEHIND the foreground, so wherever known neighbours
    differ in depth by more than depth_ratio only the farther ones are averaged.  depth_ratio = 0.05 is a convention,
    not a measurement.

    image: [N, C, H, W] or [C, H, W] device tensor (any C).  depth: [N, 1, H, W], [N, H, W] or [H, W], or None.  coverage:
    [N, H, W], [N, 1, H, W] or [H, W], or None (everything covered).  A pixel is known where coverage > 0 and, with a
    depth, 0 < z < inf; without a depth every known pixel lies at z = 1, which is plain depth-blind push-pull.  So
    warp_view's or blend_warps' dict plugs in: fill_holes(w["image"], w["depth"], w["coverage"], camera).
    camera: what the frame is an image of.  A panorama wraps in columns; a cube map's 6 S x S strip is filled as six
    independent S x S faces (nothing crosses a face border, so a face with no known pixel stays a hole); a fisheye is
    filled inside its image circle only (camera_mask) and nothing outside it is read or written; a pinhole camera or
    None is a plain image; a stereo-panorama camera raises ValueError.  levels: the number of pyramid levels above the
    frame (None: up to 1 x 1, which fills every image that has a known pixel; l levels reach about 2^l pixels into a hole).

    -> dict "image" [N, C, H, W], "depth" [N, 1, H, W] (absent when depth is None) and "filled" [N, H, W] bool: True where a
    value was written.  Known pixels keep their bits, and so does a hole that no level reaches.  The inputs are not
    modified.  Repeated calls give the same bits."""
    cam = None if camera is None else _camera(camera)
    if isinstance(cam, StereoPanoCamera):
        raise ValueError("a stereo-panorama camera is not a central projection: its frames cannot be filled")
    r = _depth_ratio(depth_ratio)
    lv = _FILL_ALL_LEVELS
    if levels is not None:
        lv = int(levels)
        if lv != levels or lv < 0:
            raise ValueError(f"levels must be a non-negative integer or None; got {levels!r}")
        lv = min(lv, _FILL_ALL_LEVELS)
    if not isinstance(image, torch.Tensor) or image.dim() not in (3, 4):
        raise ValueError(f"image must be a [C, H, W] or [N, C, H, W] tensor; got {getattr(image, 'shape', type(image))}")
    x = image.detach()
    if x.dim() == 3:
        x = x[None]
    N, C, H, W = (int(v) for v in x.shape)
    if min(N, C, H, W) < 1:
        raise ValueError("image is empty")
    if cam is not None and (H, W) != (cam.h, cam.w):
        raise ValueError(f"image is {H} x {W} but camera is {cam.h} x {cam.w}")
    if N * (C + 1) * H * W >= 1 << 31:
        raise ValueError("too many values: N (C + 1) H W must be below 2^31")
    _on_device(x, "image")
    dev = x.device
    planes = []
    for t, what in ((depth, "depth"), (coverage, "coverage")):
        if t is None:
            planes.append(None)
            continue
        ok = isinstance(t, torch.Tensor) and (tuple(t.shape) in ((N, H, W), (N, 1, H, W)) or (N == 1 and tuple(t.shape) == (H, W)))
        if not ok:
            raise ValueError(f"{what} must be [N, H, W] = {(N, H, W)}, [N, 1, H, W] or [H, W]; got {getattr(t, 'shape', type(t))}")
        _on_device(t, what)
        if t.device != dev:
            raise ValueError(f"{what} is on {t.device} but image on {dev}")
        planes.append(t.detach().reshape(N, H, W))
    z, known = planes
    cube = isinstance(cam, CubeCamera)
    n, h = (6 * N, W) if cube else (N, H)  # a cube strip is 6 N images of W x W: depth, known and filled as they lie
    with torch.no_grad(), torch.cuda.device(dev):
        out = torch.empty((N, 6, C, W, W) if cube else (N, C, H, W), dtype=torch.float32, device=dev)
        out.copy_(x.reshape(N, C, 6, W, W).permute(0, 2, 1, 3, 4) if cube else x)
        if z is not None:
            z = z.to(torch.float32, copy=True).contiguous()
        if known is not None:
            known = known.to(torch.float32).contiguous()
        domain = _domain(cam, dev) if isinstance(cam, FisheyeCamera) else None
        filled = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
        floats = int(_lib.load().pn_fill_holes_work_floats(n, C, h, W, lv))
        _lib.check(min(floats, 0), "pn_fill_holes_work_floats")
        work = torch.empty(floats, dtype=torch.float32, device=dev) if floats else None
        _lib.call("pn_fill_holes", n, C, h, W, out.data_ptr(), _lib.ptr(z), _lib.ptr(known), _lib.ptr(domain),
                  int(isinstance(cam, PanoCamera)), r, lv, filled.data_ptr(), _lib.ptr(work), floats, _lib.stream(dev))
        if cube:
            out = out.permute(0, 2, 1, 3, 4).reshape(N, C, H, W)
    res = {"image": out, "filled": filled.view(torch.bool)}
    if z is not None:
        res["depth"] = z.view(N, 1, H, W)
    return res


def render_path_warped(model, camera, poses, key_every, env_rays=None, kinds=("ldr", "depth"), near=0.0, far=10.0,
                       exposure=0.0, out_dir=None, chunk_rays=32768, max_splat=4, splat_scale=1.0, fill=0.0, blend=False,
                       inpaint=False, depth_ratio=0.05, levels=None):
    """render_path at interactive frame counts: poses 0, key_every, 2 key_every, ... and the last pose are rendered
    (render_view); every pose between two rendered poses is warp_view of those two frames (S = 2) into it.  -> render_path's
    dict of frames ("ldr" and "depth" through to_frame, "hdr" as fp32) plus "coverage" [n, H, W] fp32: 1 at a rendered
    pose and where a warped frame shows a source pixel, 0 in its holes (disocclusions, which nothing inpaints unless inpaint is set: `fill` in
    the colours, NaN in the depth - and a NaN depth anywhere makes to_frame's depth frame black, as upstream's hotmap).
    A rendered pose's frame is the render itself, so key_every = 1 gives render_path's bytes.  kinds: "ldr", "hdr", "depth"
    (what a warp carries; the others need the renderer).  With out_dir the frames go to files as render_path writes them
    and only "coverage" is returned.

    blend: every pose i between the rendered poses a < b is warped from a alone and from b alone (two warp_view calls with
    S = 1) and the two layers go through blend_warps with the weights (b - i) / (b - a) and (i - a) / (b - a), so view-
    dependent colour fades from one key to the next where both see a surface, instead of switching per pixel.  inpaint:
    the warped (or blended) frames go through fill_holes with the camera before to_frame, so their depth frames are
    complete; "coverage" still reports what the warp covered, i.e. which pixels were invented.  depth_ratio and levels
    are blend_warps' and fill_holes'.  Rendered poses are never touched; with both off these are the calls described above."""
    camera, dev, _ = _setup(model, camera, chunk_rays)
    kinds = tuple(kinds)
    bad = [k for k in kinds if k not in _WARPED_KINDS]
    if bad or not kinds:
        raise ValueError(f"kinds must be a non-empty subset of {sorted(_WARPED_KINDS)}; got {bad[0] if bad else kinds!r}")
    step = int(key_every)
    if step != key_every or step < 1:
        raise ValueError(f"key_every must be a positive integer; got {key_every!r}")
    c2ws = _c2w_stack(poses)
    n, H, W = c2ws.shape[0], camera.h, camera.w
    keys = sorted(set(range(0, n, step)) | {n - 1})
    coverage = torch.empty(n, H, W, dtype=torch.float32, device=dev)
    sink = _FrameSink(kinds, n, H, W, dev, out_dir)

    def emit(i, rgb, dep, cov):
        coverage[i].copy_(cov)
        for k in kinds:
            if k == "hdr":
                sink.put(k, i, rgb[0].permute(1, 2, 0))
            elif k == "ldr":
                sink.put(k, i, to_frame(rgb, "ldr", near, far, exposure))
            else:
                sink.put(k, i, to_frame(dep, "depth", near, far))

    def render(i):
        v = render_view(model, camera, c2ws[i], env_rays, ("rgb", "depth"), near, far, chunk_rays)
        return v["fine_rgb"], v["fine_dep"]

    one = torch.ones(H, W, dtype=torch.float32, device=dev)
    prev = render(keys[0])
    emit(keys[0], *prev, one)
    for a, b in zip(keys[:-1], keys[1:]):
        cur = render(b)
        if b - a > 1:
            if blend:  # each key frame warped alone, the two layers weighted by the distance to the other key
                ws = [warp_view(src[0], src[1], camera, c2ws[j], camera, c2ws[a + 1:b], max_splat, splat_scale, fill)
                      for src, j in ((prev, a), (cur, b))]
                wts = [[(b - i) / (b - a) for i in range(a + 1, b)], [(i - a) / (b - a) for i in range(a + 1, b)]]
                w = blend_warps(torch.stack([ws[0]["image"], ws[1]["image"]]), torch.stack([ws[0]["depth"], ws[1]["depth"]]),
                                wts, depth_ratio, fill)
            else:
                w = warp_view(torch.cat([prev[0], cur[0]]), torch.cat([prev[1], cur[1]]), camera, c2ws[[a, b]], camera,
                              c2ws[a + 1:b], max_splat, splat_scale, fill)
            if inpaint:  # coverage stays the warp's: the record of what was invented
                w = {**w, **fill_holes(w["image"], w["depth"], w["coverage"], camera, depth_ratio, levels)}
            for f, i in enumerate(range(a + 1, b)):
                emit(i, w["image"][f:f + 1], w["depth"][f:f + 1], w["coverage"][f])
        emit(b, *cur, one)
        prev = cur
    return {"coverage": coverage, **sink.frames}
