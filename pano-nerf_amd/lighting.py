"""Spatially-varying lighting of a trained model: HDR light probes, spherical harmonics and irradiance.

Pano-NeRF's field is an irradiance field: each training step estimates the light arriving at every surface point from
D golden-spiral light rays (models/pano_mip_nerf.py:319-359).  This module asks the same field for the light at any
point.  Everything runs on the HIP device through the kernels of ``libpanonerf_hip.so`` (``pn_lighting.hip`` plus the
renderer's sampling, MLP and compositing entry points), under ``torch.no_grad()`` on the current stream.  CPU tensors
raise: there is no host fallback.

    probe_directions(height, width, device)     (dirs [H W, 3], omega [H W]) of an equirectangular probe
    light_probes(model, positions, ...)         HDR radiance [P, 3, H, W] seen from each position (fine level)
    sh_project(probes)                          [P, 9, 3] real SH (l <= 2) of each probe
    irradiance(probes, normals)                 [P, K, 3] exact cosine-weighted quadrature over the probe's pixels
    sh_irradiance(sh, normals)                  [P, K, 3] Ramamoorthi-Hanrahan irradiance from SH
    field_irradiance(model, points, normals, env_rays)  [M, 3] the renderer's own shading estimate at arbitrary points
    irradiance_volume(model, bounds, resolution, ...)   IrradianceVolume(sh [nx, ny, nz, 9, 3], lo, step)
    sample_irradiance(volume, points, normals)  [M, 3] trilinear SH interpolation, then irradiance
    probes_to_cubemaps(probes, size, samples)   [P, 3, 6 size, size] cube-map strips of [P, 3, H, W] probes

Conventions (pixel directions, solid angles, SH order and constants) are stated in include/panonerf_hip.h.  Normals are
taken as given: pass unit vectors.  A probe is a plain HDR image: io_exr.write_exr writes one.
"""
import collections
import math

import numpy as np
import torch

from . import _lib, views
from .geometry import _model_device, _placement, _resolution, grid_points
from .cameras import PanoCamera
from .render import _Field, _light_gather, _planes_of

IrradianceVolume = collections.namedtuple("IrradianceVolume", ["sh", "lo", "step"])

# Ramamoorthi-Hanrahan band weights A_l per SH coefficient
_A_HAT = (math.pi,) + (2.0 * math.pi / 3.0,) * 3 + (math.pi / 4.0,) * 5
# rows per field_irradiance chunk (D Ne rows per point): as geometry's chunks, larger for the chains (~0.7 KB a row)
_ROWS_LAYERWISE = 1 << 16
_ROWS_CHAIN = 1 << 21


def _cuda(*tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"expected a tensor; got {type(t).__name__}")
        if t.device.type != "cuda":
            raise RuntimeError("pano_nerf_amd.lighting runs on a HIP device only (a tensor is on %s); there is no CPU "
                               "fallback" % t.device)
    dev = tensors[0].device
    for t in tensors[1:]:
        if t.device != dev:
            raise RuntimeError(f"tensors are on {dev} and {t.device}")
    return dev


def _size(height, width):
    h, w = int(height), int(width)
    if h < 2 or w < 2:
        raise ValueError(f"a probe needs height and width >= 2; got {height} x {width}")
    return h, w


def _table(H, W, dev):
    key = (H, W, str(dev))
    if key not in _TABLES:
        _TABLES[key] = probe_directions(H, W, dev)
    return _TABLES[key]


_TABLES = {}


def probe_directions(height, width, device=None):
    """(dirs [H W, 3], omega [H W]) fp32 on the device: the viewdirs pn_raygen_pano gives an identity camera
    (sample_dir_by_pano, utils/sampling.py:5-20; y up) and the solid angles sin((i + 1/2) pi / H) (2 pi / W) (pi / H) of
    solid_angle_refinement (utils/surface_rendering.py:294-316), evaluated in fp64 and rounded once.  Upstream's midpoint
    rule is not normalised: the omegas sum to 4 pi (1 + (pi / H)^2 / 24) approximately."""
    from .rays import generate_pano_rays
    H, W = _size(height, width)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("pano_nerf_amd.lighting runs on a HIP device only; there is no CPU fallback")
    dirs = generate_pano_rays(H, W, np.eye(4, dtype=np.float32), device=dev).viewdirs
    y = (np.arange(H) + 0.5) / H
    omega = np.sin(y * np.pi)[:, None] * (2 * np.pi / W) * (np.pi / H) * np.ones((1, W))
    return dirs, torch.from_numpy(omega.astype(np.float32).reshape(-1)).to(dev)


def _probe_view(probes):
    """(x, probe_stride, cs, ps, P, H, W) of a [P, 3, H, W] fp32 tensor read in place where its strides allow it."""
    if not isinstance(probes, torch.Tensor) or probes.dim() != 4 or probes.shape[1] != 3:
        raise ValueError(f"probes must be a [P, 3, H, W] tensor; got {getattr(probes, 'shape', type(probes))}")
    P, _, H, W = (int(s) for s in probes.shape)
    if P < 1:
        raise ValueError("probes holds no probe")
    _size(H, W)
    _cuda(probes)
    x, (sp, sc, _, sw) = views._image_view(probes)
    return x, sp, sc, sw, P, H, W


def _normals(normals, P):
    """-> (contiguous fp32 normals, K, per_probe) of [K, 3], [1, K, 3] or [P, K, 3] normals."""
    if not isinstance(normals, torch.Tensor) or normals.dim() not in (2, 3) or normals.shape[-1] != 3:
        raise ValueError(f"normals must be [K, 3], [1, K, 3] or [P, K, 3]; got {getattr(normals, 'shape', type(normals))}")
    per = normals.dim() == 3 and normals.shape[0] != 1
    if per and normals.shape[0] != P:
        raise ValueError(f"normals [{normals.shape[0]}, K, 3] do not match the {P} probes")
    K = int(normals.shape[-2])
    if K < 1:
        raise ValueError("normals holds no normal")
    return normals.detach().to(torch.float32).contiguous(), K, per


def light_probes(model, positions, height=32, width=64, near=0.0, far=10.0, chunk_rays=32768):
    """HDR radiance [P, 3, H, W] seen from each of positions [P, 3]: the fine level of the model along the rays of an
    identity-rotation equirectangular camera at the position (the rays generate_pano_rays gives, bit for bit).  Only
    the two levels run: no density-gradient sweep, no light gather.  The result is a view of a contiguous
    [P, H, W, 3] buffer."""
    P = views._probe_positions(positions)
    H, W = _size(height, width)
    dev = _cuda(positions)
    if _model_device(model) != dev:
        raise RuntimeError(f"positions are on {dev}, the model on {_model_device(model)}")
    chunk = views._chunk_rays(chunk_rays)
    out = torch.empty(P * H * W, 3, dtype=torch.float32, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        rig = views._probe_rig(positions, PanoCamera(H, W), dev)
        views._render_rows(model, rig, 0, P * H * W, None, False, False, near, far, chunk, {"fine_rgb": out}, streams=1)
    return out.view(P, H, W, 3).permute(0, 3, 1, 2)


def sh_project(probes):
    """[P, 9, 3] fp32: L_lm = sum_pix L(pix) Y_lm(dir_pix) omega_pix of each [3, H, W] probe (fp64 sums, fixed order)."""
    x, sp, sc, sw, P, H, W = _probe_view(probes)
    dev = x.device
    with torch.cuda.device(dev):
        dirs, omega = _table(H, W, dev)
        out = torch.empty(P, 9, 3, dtype=torch.float32, device=dev)
        work = torch.empty(int(_lib.load().pn_probe_sh_work_doubles(P, H, W)), dtype=torch.float64, device=dev)
        _lib.call("pn_probe_sh", P, H, W, x.data_ptr(), sp, sc, sw, dirs.data_ptr(), omega.data_ptr(), out.data_ptr(),
                  work.data_ptr(), _lib.stream(dev))
    return out


def irradiance(probes, normals):
    """[P, K, 3] fp32: E_p(n) = sum_pix L_p(pix) max(0, n . dir_pix) omega_pix, the exact quadrature over every pixel of
    each probe (upstream's shading, utils/surface_rendering.py:129-165, with the probe as the light).  normals: [K, 3]
    (or [1, K, 3]) shared by every probe, or [P, K, 3]."""
    x, sp, sc, sw, P, H, W = _probe_view(probes)
    dev = x.device
    _cuda(x, normals)
    n, K, per = _normals(normals, P)
    with torch.cuda.device(dev):
        dirs, omega = _table(H, W, dev)
        out = torch.empty(P, K, 3, dtype=torch.float32, device=dev)
        _lib.call("pn_probe_irradiance", P, H, W, x.data_ptr(), sp, sc, sw, dirs.data_ptr(), omega.data_ptr(), K,
                  n.data_ptr(), int(per), out.data_ptr(), _lib.stream(dev))
    return out


def _sh_basis(n):
    """[..., 9] real SH basis (l <= 2) at directions n [..., 3], in the header's order and constants."""
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    c0, c1, c2 = 0.28209479177387814, 0.48860251190291992, 1.0925484305920792
    c3, c4 = 0.31539156525252005, 0.54627421529603959
    return torch.stack([torch.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z),
                        c3 * (3.0 * (z * z) - 1.0), c2 * (x * z), c4 * (x * x - y * y)], -1)


def sh_irradiance(sh, normals):
    """[P, K, 3]: E(n) = sum_lm A_l L_lm Y_lm(n), A = (pi, 2 pi / 3, pi / 4) (Ramamoorthi & Hanrahan 2001), in torch
    fp32 arithmetic.  sh: [P, 9, 3]; normals: [K, 3] (or [1, K, 3]) shared, or [P, K, 3]."""
    if not isinstance(sh, torch.Tensor) or sh.dim() != 3 or tuple(sh.shape[1:]) != (9, 3):
        raise ValueError(f"sh must be a [P, 9, 3] tensor; got {getattr(sh, 'shape', type(sh))}")
    _cuda(sh, normals)
    n, K, per = _normals(normals, sh.shape[0])
    if n.dim() == 2:
        n = n[None]
    with torch.no_grad():
        a = torch.tensor(_A_HAT, dtype=torch.float32, device=sh.device)
        y = _sh_basis(n) * a  # [P or 1, K, 9]
        return torch.matmul(y.expand(sh.shape[0], -1, -1), sh.detach().to(torch.float32))


def field_irradiance(model, points, normals, env_rays, chunk_points=None):
    """[M, 3] fp32: the model's own irradiance estimate at points [M, 3] for normals [M, 3] - the renderer's `shading`
    with x_surf = points: D light rays (env_rays, as the renderer takes them) of num_env_samples samples each through
    the field, composited, cosine-weighted and summed.  Works for PanoMipNeRF and MipNeRF in every mlp_mode; a model
    built with disable_integration=True sees zero covariances, as in the renderer."""
    for name, t in (("points", points), ("normals", normals)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name} must be an [M, 3] tensor; got {getattr(t, 'shape', type(t))}")
    if points.shape[0] != normals.shape[0]:
        raise ValueError(f"{points.shape[0]} points but {normals.shape[0]} normals")
    if env_rays is None:
        raise ValueError("env_rays are required (e.g. generate_lit_rays(10, radius))")
    dev = _cuda(points, normals)
    if _model_device(model) != dev:
        raise RuntimeError(f"points are on {dev}, the model on {_model_device(model)}")
    M = int(points.shape[0])
    out = torch.empty(M, 3, dtype=torch.float32, device=dev)
    planes = _planes_of(model.mlp_mode)
    with torch.no_grad(), torch.cuda.device(dev):
        env, _ = model._env_inputs(env_rays, True, dev)  # the renderer's fp32 copies of the caller's (fp16) rays
        D = int(env[0].shape[0])
        rows = (_ROWS_CHAIN if planes else _ROWS_LAYERWISE) // (D * model.num_env_samples)
        chunk = int(chunk_points) if chunk_points else max(1, rows)
        if chunk <= 0:
            raise ValueError(f"chunk_points must be positive; got {chunk_points!r}")
        if not M:
            return out
        f = _Field.of(model, dev)
        pts = points.detach().to(torch.float32).contiguous()
        nrm = normals.detach().to(torch.float32).contiguous()
        zeros3 = torch.zeros(min(chunk, M), 3, dtype=torch.float32, device=dev)
        zeros1 = torch.zeros(min(chunk, M), dtype=torch.float32, device=dev)
        ones = torch.ones(min(chunk, M), 3, dtype=torch.float32, device=dev)  # albedo placeholder: only shading is kept
        for first in range(0, M, chunk):
            m = min(chunk, M - first)
            _, _, _, shading = _light_gather(f, pts[first:first + m], zeros3[:m], zeros1[:m], *env, None, ones[:m],
                                             nrm[first:first + m], False)
            out[first:first + m].copy_(shading)
    return out


def irradiance_volume(model, bounds, resolution, height=16, width=32, near=0.0, far=10.0, chunk_rays=32768):
    """IrradianceVolume(sh [nx, ny, nz, 9, 3], lo, step): light_probes at the vertices of a grid placed as
    geometry.density_grid places it (bounds = inclusive corner vertices, resolution = int or 3 ints, each >= 2), each
    projected onto SH.  lo / step: the fp32 placement of vertex (0, 0, 0) and the spacing."""
    res = _resolution(resolution)
    lo, step = _placement(bounds, res)
    H, W = _size(height, width)
    dev = _model_device(model)
    nv = res[0] * res[1] * res[2]
    sh = torch.empty(nv, 9, 3, dtype=torch.float32, device=dev)
    mean, _ = grid_points(bounds, res, device=dev)
    batch = max(1, (1 << 22) // (H * W))  # probes held at once (16 MB of radiance per batch)
    for first in range(0, nv, batch):
        n = min(batch, nv - first)
        sh[first:first + n] = sh_project(light_probes(model, mean[first:first + n], H, W, near, far, chunk_rays))
    return IrradianceVolume(sh.view(*res, 9, 3), lo, step)


def sample_irradiance(volume, points, normals):
    """[M, 3] fp32: irradiance at points [M, 3] for normals [M, 3] from an IrradianceVolume - the 27 coefficients
    interpolated trilinearly at the point (clamped to the box), then E(n) = sum_lm A_l L_lm Y_lm(n)."""
    sh, lo, step = volume
    if not isinstance(sh, torch.Tensor) or sh.dim() != 5 or tuple(sh.shape[3:]) != (9, 3) or min(sh.shape[:3]) < 2:
        raise ValueError(f"volume.sh must be [nx, ny, nz, 9, 3] with every axis >= 2; got {getattr(sh, 'shape', None)}")
    for name, t in (("points", points), ("normals", normals)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name} must be an [M, 3] tensor; got {getattr(t, 'shape', type(t))}")
    if points.shape[0] != normals.shape[0]:
        raise ValueError(f"{points.shape[0]} points but {normals.shape[0]} normals")
    dev = _cuda(sh, points, normals)
    M = int(points.shape[0])
    out = torch.empty(M, 3, dtype=torch.float32, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        s = sh.detach().to(torch.float32).contiguous()
        p = points.detach().to(torch.float32).contiguous()
        n = normals.detach().to(torch.float32).contiguous()
        _lib.call("pn_sh_volume_irradiance", *(int(v) for v in sh.shape[:3]), *(float(v) for v in lo),
                  *(float(v) for v in step), s.data_ptr(), M, p.data_ptr(), n.data_ptr(), out.data_ptr(), _lib.stream(dev))
    return out


def probes_to_cubemaps(probes, size, samples=4):
    """[P, 3, 6 size, size] fp32: each [3, H, W] probe as a cube map (a vertical strip of the faces +x, -x, +y, -y, +z,
    -z in the lookup convention engines use; views.cubemap_camera), every texel the mean of samples x samples bilinear
    fetches: views.reproject(probes, pano_camera(H, W), cubemap_camera(size), samples=samples)[0]."""
    _probe_view(probes)
    H, W = int(probes.shape[2]), int(probes.shape[3])
    return views.reproject(probes, views.pano_camera(H, W), views.cubemap_camera(size), samples=samples)[0]
