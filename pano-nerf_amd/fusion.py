"""TSDF fusion: posed depth images integrated into a truncated signed distance volume, and the mesh of its zero crossing.

``geometry.extract_mesh`` takes a level set of the density, which is not the surface the renderer shows and needs a level
guessed by the user.  This module is the second, independent route to a ``Mesh``: depth rendered from a handful of poses
(``render_view``'s ``fine_dep``, the renderer's expected distance that ``warp_view``, ``relight.shadow_maps`` and the
emitters use) is integrated into a signed distance volume and the zero crossing is meshed by ``marching_tetrahedra``.  It
works without a model too, on any posed depth frames of a panorama, pinhole, cube-map or fisheye camera.

The integration runs on the HIP device through ``pn_fusion.hip`` (one voxel per thread, every view inside the kernel, fp64
arithmetic, no atomics: repeated calls give the same bits), under ``torch.no_grad()`` on the current stream.  CPU tensors
raise: there is no host fallback.

    TSDFVolume(bounds, resolution, trunc)       tsdf / weight [nx, ny, nz] on geometry's grid placement
      .integrate(depth, camera, c2w, ...)       one call of pn_tsdf_integrate over S views
      .observed()                               weight > 0
      .occupancy(unknown)                       the volume marching_tetrahedra takes at level 0
      .mesh(unknown, cull)                      (vertices [V, 3], faces [F, 3] int32), wound towards free space
    fuse_views(model, camera, poses, bounds, resolution, ...)   render_view's fine_dep of every pose, integrated
    fused_mesh(model, volume | (camera, poses, bounds, resolution), ...)   geometry.Mesh with the field's normals / colours

The formulas (the signed distance along the voxel's own ray, the nearest-pixel depth, the running mean) are stated in
include/panonerf_hip.h, section "TSDF fusion".  Three conventions, not measurements: trunc = 3 x the largest grid step,
depth_max = 0.98 far in fuse_views, and unknown = "solid" (space carving).

Out of scope: colour fusion in the volume (colours come from the field, or from bake_textures on the mesh), hashed or
sparse volumes, per-pixel footprint weighting, gradients, and stereo panoramas (not a central projection).
"""
import math

import numpy as np
import torch

from . import _lib
from .cameras import StereoPanoCamera, _camera, _kind_params
from .geometry import _field_mesh, _mesh_colors, _model_device, _placement, _resolution, _variance, marching_tetrahedra
from .views import _poses, render_view

_UNKNOWN = ("solid", "empty")


def _positive(value, name, allow_inf):
    v = float(value)
    if not (v > 0.0 and (allow_inf or math.isfinite(v))):  # NaN fails too
        raise ValueError(f"{name} must be positive{'' if allow_inf else ' and finite'}; got {value!r}")
    return v


def _unknown(unknown):
    if unknown not in _UNKNOWN:
        raise ValueError(f"unknown must be 'solid' or 'empty'; got {unknown!r}")
    return unknown


def _central(camera, what):
    camera = _camera(camera)
    if isinstance(camera, StereoPanoCamera):
        raise ValueError(f"a stereo-panorama camera is not a central projection: it cannot be {what}")
    return camera


def _grid(bounds, resolution, trunc):
    """(resolution, lo, step, trunc) of a volume, lo / step / trunc as the fp32 values the kernel sees"""
    res = _resolution(resolution)
    lo, step = _placement(bounds, res)
    if not all(math.isfinite(s) and s > 0.0 for s in step) or not all(math.isfinite(v) for v in lo):
        raise ValueError(f"bounds must be finite with x0 < x1, y0 < y1, z0 < z1; got {bounds!r}")
    t = float(np.float32(3.0 * max(step) if trunc is None else _positive(trunc, "trunc", False)))
    if not (t > 0.0 and math.isfinite(t)):
        raise ValueError(f"trunc must be positive and finite in fp32; got {trunc!r}")
    return res, lo, step, t


def cull_faces(vertices, faces, observed, lo, step):
    """Drop every face whose grid cell has an unobserved corner, then the vertices no face uses; face order and relative
    vertex order are kept.  The cell of a face is c_a = min(max(floor((centroid_a - lo_a) / step_a), 0), n_a - 2) per axis,
    in fp64, with the centroid the fp64 mean of the face's fp32 vertices: this rule is the definition.  Works on torch
    tensors of any device (observed: bool [nx, ny, nz]) -> (vertices, faces int32)."""
    n = observed.shape
    v64 = vertices.to(torch.float64)
    f = faces.to(torch.int64)
    cen = (v64[f[:, 0]] + v64[f[:, 1]] + v64[f[:, 2]]) / 3.0
    lo_t = torch.tensor(lo, dtype=torch.float64, device=vertices.device)
    st_t = torch.tensor(step, dtype=torch.float64, device=vertices.device)
    c = torch.floor((cen - lo_t) / st_t)
    c = [c[:, a].clamp(0, n[a] - 2).to(torch.int64) for a in range(3)]
    cell = observed[:-1, :-1, :-1].clone()
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                cell &= observed[di:n[0] - 1 + di, dj:n[1] - 1 + dj, dk:n[2] - 1 + dk]
    keep = cell[c[0], c[1], c[2]]
    f = f[keep]
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=vertices.device)
    used[f.reshape(-1)] = True
    new = torch.cumsum(used.to(torch.int64), 0) - 1
    return vertices[used], new[f].to(torch.int32)


class TSDFVolume:
    """A truncated signed distance volume on the vertex grid of geometry.density_grid: bounds = ((x0, y0, z0), (x1, y1, z1))
    are the inclusive corner vertices, resolution an int or 3 ints (vertices per axis, each >= 2).

    tsdf [nx, ny, nz] fp32 holds the weighted mean of min(1, sdf / trunc) over the views that saw the voxel (positive in
    free space, negative behind a surface, never below -1), weight [nx, ny, nz] the summed weights; weight = 0 marks a voxel
    no view has seen, and tsdf means nothing there.  trunc is the truncation distance in world units; None gives 3 x the
    largest grid step, a convention: wide enough that every tetrahedron edge (at most sqrt(3) steps) that crosses the
    surface has both ends inside the band, narrow enough that surfaces a few voxels apart do not merge."""

    def __init__(self, bounds, resolution, trunc=None, device=None):
        self.resolution, self.lo, self.step, self.trunc = _grid(bounds, resolution, trunc)
        self.bounds = tuple(tuple(float(v) for v in c) for c in bounds)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError("pano_nerf_amd.fusion runs on a HIP device only (device=%s); there is no CPU fallback" % dev)
        if dev.index is None:  # "cuda" is the current device: tensors report their index, so hold it too
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.tsdf = torch.zeros(self.resolution, dtype=torch.float32, device=dev)
        self.weight = torch.zeros(self.resolution, dtype=torch.float32, device=dev)

    def integrate(self, depth, camera, c2w, confidence=None, weights=None, depth_max=math.inf, max_weight=math.inf):
        """Integrate S views in one call of pn_tsdf_integrate, the views in index order; returns self.

        depth: [S, 1, H, W], [S, H, W] or [H, W] device tensor, the distance t along the ray CameraRig.sample gives each
        pixel, i.e. render_view's fine_dep as it is (what warp_view takes); NaN, Inf, 0, negative depths and depths above
        depth_max are no surface.  camera: a panorama, pinhole, cube-map or fisheye camera (a stereo panorama raises
        ValueError); c2w: [S, 4, 4] (or [S, 3, 4], or one pose).  confidence: per-pixel weights shaped like depth, or None;
        weights: S per-view weights (sequence, array or tensor), or None; a weight that is not positive and finite drops
        the pixel / the view.  max_weight caps the accumulated weight, so that later views can still move an old volume.

        Every voxel reads the depth of the NEAREST pixel of its projection (interpolating across a depth discontinuity would
        invent a surface) and takes sdf = (that surface's distance) - (the voxel's distance) along its own ray; voxels more
        than trunc behind a surface are unseen by that view."""
        cam = _central(camera, "fused")
        if not isinstance(depth, torch.Tensor) or depth.dim() not in (2, 3, 4) or (depth.dim() == 4 and depth.shape[1] != 1):
            raise ValueError("depth must be a [S, 1, H, W], [S, H, W] or [H, W] tensor; got "
                             f"{getattr(depth, 'shape', type(depth))}")
        H, W = (int(v) for v in depth.shape[-2:])
        if (H, W) != (cam.h, cam.w):
            raise ValueError(f"depth is {H} x {W} but camera is {cam.h} x {cam.w}")
        z = depth.detach().reshape(-1, H, W)
        S = int(z.shape[0])
        if S < 1:
            raise ValueError("depth is empty")
        if S * H * W >= 1 << 31:
            raise ValueError("too many pixels: S H W must be below 2^31")
        conf = None
        if confidence is not None:
            if not isinstance(confidence, torch.Tensor) or confidence.numel() != z.numel() or \
                    tuple(confidence.shape[-2:]) != (H, W):
                raise ValueError(f"confidence must be shaped like depth {tuple(depth.shape)}; got "
                                 f"{getattr(confidence, 'shape', type(confidence))}")
            conf = confidence.detach().reshape(-1, H, W)
        poses = _poses(c2w, "c2w")
        if poses.shape[0] != S:
            raise ValueError(f"c2w holds {poses.shape[0]} poses but depth {S} frames")
        vw = None
        if weights is not None:
            if isinstance(weights, torch.Tensor):
                weights = weights.detach().cpu().numpy()
            vw = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1).astype(np.float32))
            if vw.shape != (S,):
                raise ValueError(f"weights must hold one weight per view ({S}); got shape {np.shape(weights)}")
        dmax = _positive(depth_max, "depth_max", True)
        wmax = _positive(max_weight, "max_weight", True)
        for t, what in ((z, "depth"), (conf, "confidence")):
            if t is not None and t.device.type != "cuda":
                raise RuntimeError("pano_nerf_amd.fusion runs on a HIP device only (the %s is on %s); there is no CPU "
                                   "fallback" % (what, t.device))
            if t is not None and t.device != self.device:
                raise ValueError(f"the {what} is on {t.device} but the volume on {self.device}")
        dev = self.device
        kind, params = _kind_params(cam)
        with torch.no_grad(), torch.cuda.device(dev):
            z = z.to(torch.float32).contiguous()
            if conf is not None:
                conf = conf.to(torch.float32).contiguous()
            up = poses.astype(np.float32).reshape(-1)
            if vw is not None:
                up = np.concatenate([up, vw])
            up = torch.from_numpy(np.ascontiguousarray(up)).to(dev)  # one upload for the poses and the view weights
            _lib.call("pn_tsdf_integrate", *self.resolution, *self.lo, *self.step, S, kind, H, W, params.ctypes.data,
                      up.data_ptr(), z.data_ptr(), _lib.ptr(conf), up[16 * S:].data_ptr() if vw is not None else None,
                      self.trunc, dmax, wmax, self.tsdf.data_ptr(), self.weight.data_ptr(), _lib.stream(dev))
        return self

    def observed(self):
        """bool [nx, ny, nz]: the voxels some view has seen (weight > 0)"""
        return self.weight > 0

    def occupancy(self, unknown="solid"):
        """The volume marching_tetrahedra takes at level 0: -tsdf where observed (inside = behind a surface); elsewhere
        +1 for unknown="solid" - the space-carving convention: what no view saw is taken as matter, which closes the mesh
        behind the surfaces - or -1 for unknown="empty"."""
        fill = 1.0 if _unknown(unknown) == "solid" else -1.0
        return torch.where(self.weight > 0, -self.tsdf, torch.full_like(self.tsdf, fill))

    def mesh(self, unknown="solid", cull=False):
        """(vertices [V, 3] fp32, faces [F, 3] int32) of the zero crossing: marching_tetrahedra(occupancy(unknown), 0,
        bounds), wound so that (v1 - v0) x (v2 - v0) points to free space.  The crossings between observed free space and
        unobserved voxels (unknown="solid") are the carved hull, not a seen surface; cull=True drops every face whose grid
        cell has an unobserved corner (cull_faces states the rule) and the vertices no face uses any more."""
        occ = self.occupancy(unknown)
        verts, faces = marching_tetrahedra(occ, 0.0, self.bounds)  # the same placement: _placement of the same bounds
        if cull and faces.shape[0]:
            with torch.no_grad(), torch.cuda.device(self.device):
                verts, faces = cull_faces(verts, faces, self.observed(), self.lo, self.step)
        return verts, faces


def fuse_views(model, camera, poses, bounds, resolution, trunc=None, env_rays=None, near=0.0, far=10.0, depth_max=None,
               confidence=None, chunk_rays=None, views_per_call=8):
    """Render the depth of every pose (render_view(..., outputs=("depth",)), its fine_dep) and integrate it into a fresh
    TSDFVolume(bounds, resolution, trunc) on the model's device, views_per_call views per integrate call; returns the volume.

    depth_max: None means 0.98 far, a convention: a ray that hits nothing reports a depth near far, and must not become
    a wall there.  confidence: [S, H, W] (or [S, 1, H, W]) per-pixel weights for all poses, or None.  chunk_rays is
    render_view's.  A stereo-panorama camera raises ValueError."""
    cam = _central(camera, "fused")
    g = int(views_per_call)
    if g != views_per_call or g < 1:
        raise ValueError(f"views_per_call must be a positive integer; got {views_per_call!r}")
    c2ws = _poses(poses, "poses")
    S = int(c2ws.shape[0])
    dmax = 0.98 * float(far) if depth_max is None else float(depth_max)
    _positive(dmax, "depth_max", True)
    if confidence is not None:
        if not isinstance(confidence, torch.Tensor) or confidence.numel() != S * cam.h * cam.w or \
                tuple(confidence.shape[-2:]) != (cam.h, cam.w):
            raise ValueError(f"confidence must be [S, H, W] = {(S, cam.h, cam.w)}; got "
                             f"{getattr(confidence, 'shape', type(confidence))}")
        confidence = confidence.reshape(S, cam.h, cam.w)
    _grid(bounds, resolution, trunc)
    vol = TSDFVolume(bounds, resolution, trunc, _model_device(model))
    kw = {} if chunk_rays is None else {"chunk_rays": chunk_rays}
    for first in range(0, S, g):
        last = min(first + g, S)
        dep = torch.cat([render_view(model, cam, c2ws[s], env_rays, ("depth",), near, far, **kw)["fine_dep"]
                         for s in range(first, last)])
        vol.integrate(dep, cam, c2ws[first:last], None if confidence is None else confidence[first:last], depth_max=dmax)
    return vol


def fused_mesh(model, *volume_or_args, normals=True, colors="auto", unknown="solid", cull=False, chunk_rows=None,
               simplify=None, min_component_faces=None, **fuse_kw):
    """geometry.Mesh(vertices, faces, normals, colors) of a fused volume: fused_mesh(model, volume) meshes a TSDFVolume,
    fused_mesh(model, camera, poses, bounds, resolution, **fuse_kw) runs fuse_views first.  Normals and colours are the
    field's at the vertices, by extract_mesh's rules (query_field with the grid's variance; colors "auto", "albedo",
    "radiance" or None), so the result goes straight into bake_textures, write_ply and write_obj.  Without a model,
    TSDFVolume.mesh() is the model-free route.  min_component_faces / simplify (a cell size or a dict of
    meshops.simplify_mesh's keywords) run meshops.clean_mesh on the mesh first - cull=True keeps every island a view
    happened to see - and the field is queried at the new vertices; with both None nothing of meshops runs."""
    colors = _mesh_colors(model, colors)
    _unknown(unknown)
    if len(volume_or_args) == 1 and isinstance(volume_or_args[0], TSDFVolume):
        if fuse_kw:
            raise ValueError(f"{sorted(fuse_kw)} belong to fuse_views; a TSDFVolume is already fused")
        vol = volume_or_args[0]
    elif len(volume_or_args) == 4:
        vol = fuse_views(model, *volume_or_args, **fuse_kw)
    else:
        raise ValueError("fused_mesh takes (model, volume) or (model, camera, poses, bounds, resolution)")
    if _model_device(model) != vol.device:
        raise RuntimeError(f"the volume is on {vol.device}, the model on {_model_device(model)}")
    verts, faces = vol.mesh(unknown, cull)
    if simplify is not None or min_component_faces is not None:
        from .meshops import clean_mesh
        verts, faces = clean_mesh(verts, faces, simplify, min_component_faces)
    return _field_mesh(model, verts, faces, float(_variance(model, None, vol.step)), normals, colors, chunk_rows)
