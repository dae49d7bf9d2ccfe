"""Light probes baked into the image-based lighting (IBL) engines consume: a GGX-prefiltered specular cube-map mip
chain, a diffuse irradiance cube and the environment-BRDF table of the split-sum approximation (Karis, "Real Shading in
Unreal Engine 4" - the paper the reference's BRDF takes its k = r^2 / 2 geometry term and spherical-Gaussian Fresnel
from, utils/surface_rendering.py:6-61).  lighting.probes_to_cubemaps was the first half of the export; this is the second.

Everything runs on the HIP device through the kernels of ``libpanonerf_hip.so`` (``pn_ibl.hip``), under
``torch.no_grad()`` on the current stream.  CPU tensors raise: there is no host fallback.  Every sum is fp64 in a fixed
order on fp32 inputs, rounded once per output: repeated calls give the same bits.

    prefilter(probes, directions, roughness)    [P, K, 3] GGX-prefiltered radiance around each direction (N = V = R)
    prefilter_cubemaps(probes, size, levels)    ([P, 3, 6 S_l, S_l] per level, roughness per level)
    irradiance_cubemaps(probes, size)           [P, 3, 6 size, size] lighting.irradiance at the texel directions
    brdf_lut(size, samples)                     [size, size, 2] (A, B): specular = prefiltered (F0 A + B)
    bake_ibl(probes, ...)                       IBL(specular, roughness, irradiance, lut)
    save_ibl(ibl, out_dir, probe)               EXR strips, the table and ibl.json
    ibl_shade(ibl, albedo, normals, viewdirs, roughness)   (rgb, diffuse, specular): what an engine shows

Formulas and conventions are stated in include/panonerf_hip.h; cube maps are vertical strips of the faces +x, -x, +y, -y,
+z, -z in the lookup convention (views.cubemap_camera).  Directions and normals are taken as given: pass unit vectors.
"""
import collections
import json
import math
import os

import numpy as np
import torch

from . import _lib
from .lighting import _cuda, _normals, _probe_view, _table, irradiance, probes_to_cubemaps

IBL = collections.namedtuple("IBL", ["specular", "roughness", "irradiance", "lut"])
FACES = ("+x", "-x", "+y", "-y", "+z", "-z")

_TEXELS = {}


def _texel_directions(size, dev):
    """[6 size size, 3] fp32: the viewdirs generate_camera_rays gives cubemap_camera(size) at the identity pose."""
    key = (int(size), str(dev))
    if key not in _TEXELS:
        from . import views
        _TEXELS[key] = views.generate_camera_rays(views.cubemap_camera(size), np.eye(4, dtype=np.float32),
                                                  device=dev).viewdirs.contiguous()
    return _TEXELS[key]


def _roughness(roughness):
    r = float(roughness)
    if not 0.0 < r <= 1.0:
        raise ValueError(f"roughness must lie in (0, 1] (at 0 the lobe is a delta: use the probe itself); got {roughness!r}")
    return r


def _pow2(size, least, what):
    s = int(size)
    if s != size or s < least or s & (s - 1):
        raise ValueError(f"{what} must be a power of two >= {least}; got {size!r}")
    return s


def _levels(size, levels):
    top = size.bit_length() - 1  # log2(size)
    n = top - 1 if levels is None else int(levels)
    if (levels is not None and n != levels) or not 2 <= n <= top + 1:
        raise ValueError(f"levels must be an integer in [2, {top + 1}] for size {size}; got {levels!r}")
    return n


def _strips(x, size):
    """[P, K = 6 size size, 3] -> the [P, 3, 6 size, size] view."""
    return x.view(x.shape[0], 6 * size, size, 3).permute(0, 3, 1, 2)


def prefilter(probes, directions, roughness):
    """[P, K, 3] fp32: the GGX-prefiltered radiance of each [3, H, W] probe around each unit direction n under the
    split-sum assumption N = V = R, a deterministic quadrature over every probe pixel (direction d, solid angle omega,
    radiance L), not Monte Carlo.  With alpha = roughness^2:
        c = max(0, n . d),  den = (1 + c) / 2 (alpha^2 - 1) + 1,  w = c omega / den^2,  out = sum w L / sum w
    roughness: one float in (0, 1].  directions: [K, 3] (or [1, K, 3]) shared by every probe, or [P, K, 3].  A probe's
    result does not depend on P.  NaN radiance makes its channel NaN for every direction of the probe, as in
    lighting.irradiance."""
    r = _roughness(roughness)
    x, sp, sc, sw, P, H, W = _probe_view(probes)
    dev = x.device
    _cuda(x, directions)
    n, K, per = _normals(directions, P)
    with torch.no_grad(), torch.cuda.device(dev):
        dirs, omega = _table(H, W, dev)
        out = torch.empty(P, K, 3, dtype=torch.float32, device=dev)
        work = torch.empty(int(_lib.load().pn_prefilter_work_doubles(P, H, W, K)), dtype=torch.float64, device=dev)
        _lib.call("pn_prefilter", P, H, W, x.data_ptr(), sp, sc, sw, dirs.data_ptr(), omega.data_ptr(), K, n.data_ptr(),
                  int(per), r, out.data_ptr(), work.data_ptr(), _lib.stream(dev))
    return out


def prefilter_cubemaps(probes, size, levels=None, samples=4, allow_coarse=False):
    """-> (list of `levels` tensors [P, 3, 6 S_l, S_l], S_l = size >> l, tuple of roughness r_l = l / (levels - 1)): the
    specular mip chain in which roughness selects the level.  Level 0 is probes_to_cubemaps(probes, size, samples);
    level l >= 1 is prefilter at the texel-centre directions of cubemap_camera(S_l) (views of [P, 6 S_l, S_l, 3]
    buffers).  size: a power of two >= 4; levels: 2 .. log2(size) + 1, by default log2(size) - 1 (the smallest level is
    4 x 4).  The quadrature cannot resolve a lobe narrower than its pixels: ValueError when pi / H > r_1^2 (the pixel
    spacing against the lobe width alpha of the sharpest filtered level) unless allow_coarse=True."""
    S = _pow2(size, 4, "size")
    n = _levels(S, levels)
    x, _, _, _, P, H, W = _probe_view(probes)
    rough = tuple(l / (n - 1) for l in range(n))
    if math.pi / H > rough[1] ** 2 and not allow_coarse:
        raise ValueError(f"a {H} x {W} probe cannot resolve the GGX lobe of level 1 (roughness {rough[1]:.3g}: pi / H = "
                         f"{math.pi / H:.3g} > roughness^2 = {rough[1] ** 2:.3g}); render larger probes, use fewer levels "
                         "or pass allow_coarse=True")
    out = [probes_to_cubemaps(probes, S, samples)]
    for l in range(1, n):
        out.append(_strips(prefilter(probes, _texel_directions(S >> l, x.device), rough[l]), S >> l))
    return out, rough


def irradiance_cubemaps(probes, size):
    """[P, 3, 6 size, size] fp32: lighting.irradiance of each probe at the texel-centre directions of
    cubemap_camera(size), the diffuse cube an engine multiplies by albedo / pi (a view of a [P, 6 size, size, 3] buffer)."""
    S = int(size)
    if S != size or S < 2:
        raise ValueError(f"a cube map needs an integer size >= 2; got {size!r}")
    x = _probe_view(probes)[0]
    return _strips(irradiance(probes, _texel_directions(S, x.device)), S)


def brdf_lut(size=32, samples=256, device=None):
    """[size, size, 2] fp32 (A, B) of the split-sum environment BRDF: specular = prefiltered (F0 A + B).  Row i is
    roughness (i + 1/2) / size, column j is NoV (j + 1/2) / size; the reference's geometry term (k = r^2 / 2) and
    spherical-Gaussian Fresnel, a midpoint rule on a samples x samples GGX-warped grid in fp64.  The rule is first order
    at grazing NoV (the hard NoL > 0 cut): on a 16 x 16 table the largest change from 128 to 512 samples is 0.009, at
    NoV = 1 / 32; the default 256 lies between.  The table carries the cosine NoL an engine expects."""
    S, n = int(size), int(samples)
    if S != size or not 2 <= S <= 4096:
        raise ValueError(f"size must be an integer in [2, 4096]; got {size!r}")
    if n != samples or not 1 <= n <= 4096:
        raise ValueError(f"samples must be an integer in [1, 4096]; got {samples!r}")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("pano_nerf_amd.ibl runs on a HIP device only; there is no CPU fallback")
    with torch.no_grad(), torch.cuda.device(dev):
        out = torch.empty(S, S, 2, dtype=torch.float32, device=dev)
        _lib.call("pn_brdf_lut", S, n, out.data_ptr(), _lib.stream(dev))
    return out


def bake_ibl(probes, size=32, levels=None, irradiance_size=8, lut_size=32, samples=4, lut_samples=256, allow_coarse=False):
    """IBL(specular, roughness, irradiance, lut) of [P, 3, H, W] probes: prefilter_cubemaps(probes, size, levels,
    samples), irradiance_cubemaps(probes, irradiance_size) and brdf_lut(lut_size, lut_samples).  The table does not
    depend on the probes and is half the cost of a small bake: who bakes many batches builds the IBL from the three
    parts and keeps one table."""
    specular, rough = prefilter_cubemaps(probes, size, levels, samples, allow_coarse)
    return IBL(specular, rough, irradiance_cubemaps(probes, irradiance_size),
               brdf_lut(lut_size, lut_samples, specular[0].device))


def _ibl(ibl, probe):
    """-> (specular list, irradiance, lut, size, levels, probe) of a checked IBL."""
    if not isinstance(ibl, IBL):
        raise ValueError(f"ibl must come from bake_ibl; got {type(ibl).__name__}")
    specular, rough, irr, lut = ibl
    n = len(specular)
    if n < 2 or len(rough) != n:
        raise ValueError(f"an IBL holds at least 2 specular levels and a roughness per level; got {n} and {len(rough)}")
    dev = _cuda(*specular, irr, lut)
    P, size = int(specular[0].shape[0]), int(specular[0].shape[3])
    for l, t in enumerate(specular):
        if tuple(t.shape) != (P, 3, 6 * (size >> l), size >> l) or not size >> l:
            raise ValueError(f"specular level {l} must be [{P}, 3, {6 * (size >> l)}, {size >> l}]; got {tuple(t.shape)}")
    if irr.dim() != 4 or tuple(irr.shape[:2]) != (P, 3) or irr.shape[2] != 6 * irr.shape[3]:
        raise ValueError(f"irradiance must be [{P}, 3, 6 S, S]; got {tuple(irr.shape)}")
    if lut.dim() != 3 or lut.shape[0] != lut.shape[1] or lut.shape[2] != 2 or lut.shape[0] < 2:
        raise ValueError(f"lut must be [S, S, 2] with S >= 2; got {tuple(lut.shape)}")
    p = int(probe)
    if p != probe or not 0 <= p < P:
        raise IndexError(f"probe {probe!r} is out of range for {P} probes")
    return specular, irr, lut, size, n, p, dev


def save_ibl(ibl, out_dir, probe=0):
    """Write one probe's assets to out_dir as uncompressed FLOAT OpenEXR (io_exr.write_exr): specular_l{l}.exr (the
    6 S_l x S_l strips), irradiance.exr, brdf_lut.exr (A in R, B in G, 0 in B) and ibl.json (sizes, roughness per level,
    face order, file names).  -> the path of ibl.json."""
    from . import io_exr
    specular, irr, lut, size, n, p, _ = _ibl(ibl, probe)
    os.makedirs(out_dir, exist_ok=True)

    def hwc(t):
        return np.ascontiguousarray(t[p].detach().to(torch.float32).permute(1, 2, 0).cpu().numpy())

    names = [f"specular_l{l}.exr" for l in range(n)]
    for name, t in zip(names, specular):
        io_exr.write_exr(os.path.join(out_dir, name), hwc(t))
    io_exr.write_exr(os.path.join(out_dir, "irradiance.exr"), hwc(irr))
    table = lut.detach().to(torch.float32).cpu().numpy()
    io_exr.write_exr(os.path.join(out_dir, "brdf_lut.exr"),
                     np.ascontiguousarray(np.concatenate([table, np.zeros_like(table[:, :, :1])], axis=2)))
    meta = dict(probe=p, faces=list(FACES), layout="vertical strip, 6 size rows x size columns",
                specular=[dict(file=name, size=size >> l, roughness=float(ibl.roughness[l])) for l, name in enumerate(names)],
                irradiance=dict(file="irradiance.exr", size=int(irr.shape[3])),
                brdf_lut=dict(file="brdf_lut.exr", size=int(lut.shape[0]), channels=["A", "B", "0"],
                              rows="roughness (i + 1/2) / size", columns="NoV (j + 1/2) / size"))
    path = os.path.join(out_dir, "ibl.json")
    with open(path, "w") as f:
        json.dump(meta, f, indent=1)
    return path


def ibl_shade(ibl, albedo, normals, viewdirs, roughness, f0=0.04, probe=0):
    """(rgb, diffuse, specular), each [R, 3] fp32: an engine's split-sum evaluation of rows with albedo, unit normals and
    viewdirs [R, 3] (camera to surface, as everywhere here) under probe `probe` of a baked IBL.  roughness: a float or
    [R, 1].  With v = -viewdirs / |viewdirs|, NoV = max(0, n . v), Rr = 2 (n . v) n - v:
        light = the specular chain at Rr, trilinear at level clamp(roughness (levels - 1), 0, levels - 1)
        E = the irradiance cube at n,  (A, B) = the table at (NoV, roughness), bilinear
        diffuse = albedo / pi E,  specular = light (f0 A + B),  rgb = diffuse + specular
    Fetches are bilinear and clamp within the face, as views.reproject.  The table carries NoL, which the reference's
    specular sum omits: this is what an engine will show, not an approximation of objects.shade."""
    specular, irr, lut, size, n, p, dev = _ibl(ibl, probe)
    for name, t in (("albedo", albedo), ("normals", normals), ("viewdirs", viewdirs)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name} must be an [R, 3] tensor; got {getattr(t, 'shape', type(t))}")
    R = int(albedo.shape[0])
    if normals.shape[0] != R or viewdirs.shape[0] != R:
        raise ValueError(f"{R} albedo rows but {normals.shape[0]} normals and {viewdirs.shape[0]} viewdirs")
    _cuda(lut, albedo, normals, viewdirs)
    rough_t, rough_all = None, 0.0
    if isinstance(roughness, torch.Tensor):
        if tuple(roughness.shape) not in ((R, 1), (R,)):
            raise ValueError(f"roughness must be a float or [R, 1]; got {tuple(roughness.shape)}")
        _cuda(lut, roughness)
        rough_t = roughness.detach().to(torch.float32).contiguous()
    else:
        rough_all = float(roughness)
    with torch.no_grad(), torch.cuda.device(dev):
        a, nrm, vd = (t.detach().to(torch.float32).contiguous() for t in (albedo, normals, viewdirs))
        chain = torch.cat([t[p].detach().to(torch.float32).reshape(-1) for t in specular])
        e = irr[p].detach().to(torch.float32).contiguous()
        table = lut.detach().to(torch.float32).contiguous()
        rgb, diffuse, spec = (torch.empty(R, 3, dtype=torch.float32, device=dev) for _ in range(3))
        _lib.call("pn_ibl_shade", R, size, n, chain.data_ptr(), int(irr.shape[3]), e.data_ptr(), int(lut.shape[0]),
                  table.data_ptr(), a.data_ptr(), nrm.data_ptr(), vd.data_ptr(), _lib.ptr(rough_t), rough_all, float(f0),
                  rgb.data_ptr(), diffuse.data_ptr(), spec.data_ptr(), _lib.stream(dev))
    return rgb, diffuse, spec
