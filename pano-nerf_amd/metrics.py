"""Validation metrics of a rendered panorama (host-side torch ops on whatever device the image lives on).

Mirrors the functions `systems/panonerf_system.py:validation_step` calls from `utils/metrics.py`:
`calc_mse/rmse/l1/psnr` (:210-237), `calc_mae` / `calc_cossimi` (:240-257) and the solid-angle weighted family
`calc_ws_psnr/l1/mse/rmse/mae/cossimi` (:318-397) with `solid_angle_refinement` (`utils/surface_rendering.py:294-316`).
An equirectangular pixel in row i covers sin(phi_i) dtheta dphi steradians, so the weights are sin((i + .5) pi / H),
normalised to sum 1.  Not part of the training hot path; SURVEY.md 8f rank 4.

The rest of the reference's metrics (`calc_ssim` / `ssim` :44-200, the depth metrics :290-315, `calc_simse` :400-404),
`calc_ws_ssim` (ours) and `evaluate_panorama` (one call that scores a `render_image` output) run on the HIP kernels of
`csrc/pn_metrics.hip` when their inputs are CUDA tensors and as host-torch restatements (fp64 sums) otherwise.
The kernels only enqueue work: the functions return 0-d device tensors without a host sync, and `evaluate_panorama`
copies a few dozen doubles back once.  Parity of the EXR writer with the OpenEXR library stays unpinned.
"""
import math

import torch
import torch.nn.functional as F

from . import _lib


def solid_angle_refinement(h=8, w=16, hemisp=False, device=None):
    """[1, h*w, 1] steradians per pixel of an h x w equirectangular image (upper hemisphere only if `hemisp`)."""
    phi_range = math.pi / 2 if hemisp else math.pi
    rows = (torch.arange(h, dtype=torch.float64) + 0.5) / h
    sa = torch.sin(rows * phi_range) * (2 * math.pi / w) * (phi_range / h)
    return sa.reshape(h, 1).expand(h, w).reshape(1, -1, 1).to(torch.float32).to(device)


def _weights(h, w, device):
    wt = solid_angle_refinement(h, w, device=device).reshape(1, h, w)
    return wt / wt.sum()


def calc_mse(x, y):
    return torch.mean((x - y) ** 2)


def calc_rmse(x, y):
    return torch.mean((x - y) ** 2) ** 0.5


def calc_l1(x, y):
    return torch.abs(x - y).mean()


def calc_psnr(x, y):
    return -10.0 * torch.log10(calc_mse(x, y))


def _angles(x, y, dim):
    if dim == 1:
        x, y = x.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1)
    cos = F.cosine_similarity(x.reshape(-1, 3), y.reshape(-1, 3), dim=-1)
    return torch.nan_to_num(torch.acos(cos) / math.pi * 180, nan=0.0), x


def calc_mae(x, y, dim=-1):
    """Mean angular error in degrees between two [B,H,W,3] (dim=-1) or [B,3,H,W] (dim=1) vector images."""
    return _angles(x, y, dim)[0].mean()


def calc_cossimi(x, y, dim=-1):
    return F.cosine_similarity(x, y, dim=dim).mean()


def calc_ws_mse(pred, gt):
    """Solid-angle weighted squared error of [C,H,W] images (summed over channels, as upstream)."""
    _, h, w = pred.shape
    return torch.sum((pred - gt) ** 2 * _weights(h, w, pred.device))


def calc_ws_rmse(pred, gt):
    return torch.sqrt(calc_ws_mse(pred, gt))


def calc_ws_psnr(pred, gt):
    return -10.0 * torch.log10(calc_ws_mse(pred, gt))


def calc_ws_l1(pred, gt):
    _, h, w = pred.shape
    return torch.sum(torch.abs(pred - gt) * _weights(h, w, pred.device))


def calc_ws_mae(x, y, dim=-1, weights=None):
    ang, xp = _angles(x, y, dim)
    if weights is None:
        _, h, w, _ = xp.shape
        weights = solid_angle_refinement(h, w, device=x.device)
    weights = weights.reshape(-1).to(x.device)
    return torch.sum(ang * (weights / weights.sum()))


def calc_ws_cossimi(x, y, dim=0):
    if dim == 0:
        _, h, w = x.shape
    elif dim == -1:
        h, w, _ = x.shape
    elif dim == 1:
        _, _, h, w = x.shape
    else:
        raise ValueError("dim must be 0, 1 or -1")
    cos = F.cosine_similarity(x, y, dim=dim).reshape(1, h, w)
    return torch.sum(cos * _weights(h, w, x.device))


# ---- the evaluation path: HIP kernels on CUDA tensors, host-torch restatements (fp64) otherwise ---------------------
# Each `_*_sums` returns the fp64 sums of one kernel of csrc/pn_metrics.hip (layout in include/panonerf_hip.h) and each
# metric is derived from them by the same tensor expression on either path.

TONE_NONE, TONE_LDR, TONE_LDR_U8 = 0, 1, 2  # hdr_to_ldr off / hdr_to_ldr(x) / hdr_to_ldr(x, dtype='uint8')
_N_SUMS, _N_SSIM, _N_NORMALS, _N_DEPTH = 6, 3, 5, 9
_DELTA_DEGREES = (1, 2, 3)
_EPS_LOG = float(torch.tensor(1e-7, dtype=torch.float32))  # torch compares fp32 depths with the scalar cast to fp32


def _tonemap(x, mode):
    """hdr_to_ldr (utils/surface_rendering.py:319-341) evaluated on fp32 values as the reference does (the uint8
    truncation is defined on them), returned in x's dtype."""
    if mode == TONE_NONE:
        return x
    if mode not in (TONE_LDR, TONE_LDR_U8):
        raise ValueError(f"unknown tone mapping mode {mode}")
    c = x.to(torch.float32)
    c = torch.clamp((c * (2.51 * c + 0.03)) / (c * (2.43 * c + 0.59) + 0.14), 0, 1)
    if mode == TONE_LDR_U8:
        c = torch.trunc(c * 255.0) / 255.0
    return (c ** (1 / 2.2)).to(x.dtype)


def _chw(t):
    """[C, H, W] view of a [C, H, W] or [1, C, H, W] image."""
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3:
        raise ValueError(f"expected a [C, H, W] or [1, C, H, W] image, got shape {tuple(t.shape)}")
    return t


def _row_weights(h, w):
    """[H, 1] fp64 solid-angle weight of one pixel of each row, summing to 1 over the H x W image."""
    rows = torch.sin((torch.arange(h, dtype=torch.float64) + 0.5) * math.pi / h)
    return (rows / (rows.sum() * w)).reshape(h, 1)


def _count(t):
    return torch.tensor(float(t.numel()), dtype=torch.float64)


def _cuda(*ts):
    return any(t is not None and t.is_cuda for t in ts)


def _device(*ts):
    return next(t.device for t in ts if t is not None and t.is_cuda)


def _planes(t):
    """(tensor, C, H, W, channel stride, pixel stride) of an fp32 CUDA image, read in place whenever its H and W
    dimensions collapse into one pixel index (as in the permuted [1, C, H, W] views render_image returns)."""
    t = _chw(t)
    if t.dtype != torch.float32:
        t = t.float()
    c, h, w = t.shape
    if w == 1:
        ps = t.stride(1)
    elif h == 1 or t.stride(1) == w * t.stride(2):
        ps = t.stride(2)
    else:
        t = t.contiguous()
        ps = 1
    return t, c, h, w, t.stride(0), ps


def _flat(t):
    """(tensor, element stride) of an fp32 CUDA tensor read as one strided run of elements."""
    t = t.float().reshape(-1)
    return t, t.stride(0)


def _workspace(dev, c, h, w):
    n = _lib.load().pn_metrics_work_doubles(c, h, w)
    _lib.check(min(int(n), 0), "pn_metrics_work_doubles")
    return torch.empty(int(n), dtype=torch.float64, device=dev)


def _pair(x, y):
    dev = _device(x, y)
    xt, c, h, w, xcs, xps = _planes(x.to(dev))
    yt, *shape, ycs, yps = _planes(y.to(dev))
    if list(shape) != [c, h, w]:
        raise ValueError(f"image shapes differ: {(c, h, w)} and {tuple(shape)}")
    return (xt, xcs, xps), (yt, ycs, yps), (c, h, w)


def _image_sums(x, y, tx=TONE_NONE, ty=TONE_NONE, out=None, work=None):
    """[sum d^2, sum |d|, sum w d^2, sum w |d|, sum d, count] of d = tone(x) - tone(y) over [C, H, W] images."""
    if _cuda(x, y):
        (xt, xcs, xps), (yt, ycs, yps), (c, h, w) = _pair(x, y)
        dev = xt.device
        out = torch.empty(_N_SUMS, dtype=torch.float64, device=dev) if out is None else out
        work = _workspace(dev, c, h, w) if work is None else work
        _lib.call("pn_metric_sums", c, h, w, xt.data_ptr(), xcs, xps, tx, yt.data_ptr(), ycs, yps, ty, out.data_ptr(),
                  work.data_ptr(), _lib.stream(dev))
        return out
    a, b = _chw(x), _chw(y)
    d = _tonemap(a, tx).double() - _tonemap(b, ty).double()
    wt = _row_weights(d.shape[1], d.shape[2])
    d2, ad = d * d, d.abs()
    return torch.stack([d2.sum(), ad.sum(), (wt * d2).sum(), (wt * ad).sum(), d.sum(), _count(d)])


def _gaussian_taps(window_size):
    """utils/metrics.py:9-16: fp32 exp(-(k - r)^2 / (2 * 1.5^2)) over its fp32 sum."""
    g = torch.exp(torch.tensor([-(k - window_size // 2) ** 2 / float(2 * 1.5 ** 2) for k in range(window_size)]))
    return g / g.sum()


_DEVICE_TAPS = {}  # device -> the fp64 copy of _gaussian_taps(11) the SSIM kernel reads (built once per device)


def _device_taps(dev):
    if dev not in _DEVICE_TAPS:
        _DEVICE_TAPS[dev] = _gaussian_taps(11).double().to(dev)
    return _DEVICE_TAPS[dev]


def _ssim_sums(x, y, tx=TONE_NONE, ty=TONE_NONE, window_size=11, max_val=1.0, want_map=False, out=None, work=None):
    """([sum s, sum w s (over channels), count], SSIM map [C, H, W] or None) of tone(x) and tone(y)."""
    if _cuda(x, y):
        (xt, xcs, xps), (yt, ycs, yps), (c, h, w) = _pair(x, y)
        dev = xt.device
        out = torch.empty(_N_SSIM, dtype=torch.float64, device=dev) if out is None else out
        work = _workspace(dev, c, h, w) if work is None else work
        smap = torch.empty(c, h, w, dtype=torch.float32, device=dev) if want_map else None
        _lib.call("pn_metric_ssim", c, h, w, xt.data_ptr(), xcs, xps, tx, yt.data_ptr(), ycs, yps, ty, int(window_size),
                  _device_taps(dev).data_ptr(), float(max_val), _lib.ptr(smap), out.data_ptr(), work.data_ptr(),
                  _lib.stream(dev))
        return out, smap
    a = _tonemap(_chw(x), tx).double()[:, None]
    b = _tonemap(_chw(y), ty).double()[:, None]
    g, r = _gaussian_taps(window_size).double(), window_size // 2

    def blur(v):  # the 2-D window is the outer product of the taps: two 1-D zero-padded passes
        return F.conv2d(F.conv2d(v, g.view(1, 1, 1, -1), padding=(0, r)), g.view(1, 1, -1, 1), padding=(r, 0))

    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    mu1, mu2 = blur(a), blur(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = blur(a * a) - mu1_sq, blur(b * b) - mu2_sq, blur(a * b) - mu1_mu2
    smap = (((2 * mu1_mu2 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s11 + s22 + c2)))[:, 0]
    wt = _row_weights(smap.shape[1], smap.shape[2])
    return torch.stack([smap.sum(), (wt * smap).sum(), _count(smap)]), (smap if want_map else None)


def _normal_sums(x, y, y_normalize=0, out=None, work=None):
    """[sum angle, sum w angle, sum cos, sum w cos, count] of two [3, H, W] normal images; y first goes through
    `y_normalize` passes of F.normalize."""
    if _cuda(x, y):
        (xt, xcs, xps), (yt, ycs, yps), (c, h, w) = _pair(x, y)
        if c != 3:
            raise ValueError("normal images have 3 channels")
        dev = xt.device
        out = torch.empty(_N_NORMALS, dtype=torch.float64, device=dev) if out is None else out
        work = _workspace(dev, 3, h, w) if work is None else work
        _lib.call("pn_metric_normals", h, w, xt.data_ptr(), xcs, xps, yt.data_ptr(), ycs, yps, int(y_normalize),
                  out.data_ptr(), work.data_ptr(), _lib.stream(dev))
        return out
    a, b = _chw(x), _chw(y)
    for _ in range(y_normalize):
        b = F.normalize(b, dim=0)
    cos = F.cosine_similarity(a, b, dim=0)
    ang = torch.nan_to_num(torch.acos(cos.double()) * (180 / math.pi), nan=0.0)
    cos = cos.double()
    wt = _row_weights(cos.shape[0], cos.shape[1])
    return torch.stack([ang.sum(), (wt * ang).sum(), cos.sum(), (wt * cos).sum(), _count(cos)])


def _depth_sums(pred, gt, mask=None, out=None, work=None):
    """[count, sum |d|/g, sum d^2/g, sum d^2, log count, sum (log p - log g)^2, delta_1..3 counts] over mask > 0."""
    if pred.numel() != gt.numel() or (mask is not None and mask.numel() != pred.numel()):
        raise ValueError("pred, gt and mask must have the same number of elements")
    if _cuda(pred, gt, mask):
        dev = _device(pred, gt, mask)
        (p, ps), (g, gs) = _flat(pred.to(dev)), _flat(gt.to(dev))
        m, ms = _flat(mask.to(dev)) if mask is not None else (None, 0)
        out = torch.empty(_N_DEPTH, dtype=torch.float64, device=dev) if out is None else out
        work = _workspace(dev, 1, 1, 1) if work is None else work
        _lib.call("pn_metric_depth", p.numel(), p.data_ptr(), ps, g.data_ptr(), gs, _lib.ptr(m), ms, out.data_ptr(),
                  work.data_ptr(), _lib.stream(dev))
        return out
    p, g = pred.reshape(-1).double(), gt.reshape(-1).double()
    if mask is not None:
        sel = mask.reshape(-1) > 0
        p, g = p[sel], g[sel]
    d = p - g
    ok = (p > _EPS_LOG) & (g > _EPS_LOG)
    lg = p[ok].log() - g[ok].log()
    r1, r2 = p / g, g / p
    inl = [((r1 < 1.25 ** k) & (r2 < 1.25 ** k)).double().sum() for k in _DELTA_DEGREES]
    return torch.stack([_count(d), (d.abs() / g).sum(), (d * d / g).sum(), (d * d).sum(), _count(lg), (lg * lg).sum()]
                       + inl)


# derived metrics (torch semantics: an empty selection gives 0 / 0 = NaN)
def _mse(s):
    return s[0] / s[5]


def _psnr(s):
    return -10.0 * torch.log10(_mse(s))


def _ws_psnr(s):
    return -10.0 * torch.log10(s[2])


def _simse(s):
    return (s[0] - s[4] * s[4] / s[5]) / (s[5] - 1)  # torch.var: unbiased


def _depth_metric(s, name, degree=1):
    if name == "abs_rel":
        return s[1] / s[0]
    if name == "sq_rel":
        return s[2] / s[0]
    if name == "lin_rms":
        return torch.sqrt(s[3] / s[0])
    if name == "log_rms":
        return torch.sqrt(s[5] / s[4])
    return s[5 + degree] / s[0]


def ssim(img1, img2, window_size=11, reduction="none", max_val=1.0):
    """utils/metrics.py:172-187: SSIM of [B, C, H, W] images (11 x 11 Gaussian window, sigma 1.5, zero padding) with
    reduction 'none' (the [B, C, H, W] map), 'mean' or 'sum'.  The kernel supports window_size 11 only."""
    if reduction not in ("none", "mean", "sum"):
        raise ValueError(f"unknown reduction {reduction!r}")
    if img1.dim() != 4 or img1.shape != img2.shape:
        raise ValueError(f"expected two [B, C, H, W] images of one shape, got {tuple(img1.shape)}, {tuple(img2.shape)}")
    parts = [_ssim_sums(img1[b], img2[b], window_size=window_size, max_val=max_val, want_map=reduction == "none")
             for b in range(img1.shape[0])]
    if reduction == "none":
        return torch.stack([m for _, m in parts]).to(img1.dtype)
    s = torch.stack([v for v, _ in parts]).sum(0)
    return (s[0] / s[2] if reduction == "mean" else s[0]).to(img1.dtype)


def calc_ssim(x, y):
    """utils/metrics.py:190-195: mean SSIM of [B, C, H, W] images."""
    return ssim(x, y, window_size=11, reduction="mean")


def calc_ws_ssim(x, y, max_val=1.0):
    """Solid-angle-weighted mean SSIM of [C, H, W] or [B, C, H, W] panoramas: the SSIM map weighted by the pixel solid
    angles (normalised to sum 1 per channel) and averaged over channels and batch.  Not in the reference: the standard
    360-degree form of SSIM, added here next to calc_ws_psnr."""
    xs = x if x.dim() == 4 else x[None]
    ys = y if y.dim() == 4 else y[None]
    s = torch.stack([_ssim_sums(a, b, max_val=max_val)[0] for a, b in zip(xs, ys)]).sum(0)
    return (s[1] * (x.shape[-1] * x.shape[-2]) / s[2]).to(x.dtype)


def abs_rel_error(pred, gt, mask=None):
    """utils/metrics.py:290-292 (mask None: every element)."""
    return _depth_metric(_depth_sums(pred, gt, mask), "abs_rel").to(pred.dtype)


def sq_rel_error(pred, gt, mask=None):
    """utils/metrics.py:295-297."""
    return _depth_metric(_depth_sums(pred, gt, mask), "sq_rel").to(pred.dtype)


def lin_rms_sq_error(pred, gt, mask=None):
    """utils/metrics.py:300-302: the square root IS taken, despite the name."""
    return _depth_metric(_depth_sums(pred, gt, mask), "lin_rms").to(pred.dtype)


def log_rms_sq_error(pred, gt, mask=None):
    """utils/metrics.py:305-308: over mask > 0 with pred > 1e-7 and gt > 1e-7 (square root taken)."""
    return _depth_metric(_depth_sums(pred, gt, mask), "log_rms").to(pred.dtype)


def delta_inlier_ratio(pred, gt, mask=None, degree=1):
    """utils/metrics.py:311-313: share of max(pred / gt, gt / pred) < 1.25 ** degree, degree 1, 2 or 3."""
    if degree not in _DELTA_DEGREES:
        raise ValueError(f"degree must be one of {_DELTA_DEGREES}")
    return _depth_metric(_depth_sums(pred, gt, mask), "delta", degree).to(pred.dtype)


def calc_simse(x, y):
    """utils/metrics.py:400-404: torch.var(x - y) (unbiased), from one pass of fp64 sums."""
    planar = x.dim() == 3 or (x.dim() == 4 and x.shape[0] == 1)
    if not (planar and x.shape == y.shape and x.shape[-3] in (1, 3)):
        x, y = x.reshape(1, 1, -1), y.reshape(1, 1, -1)  # any other shape: one channel of one row
    return _simse(_image_sums(x, y)).to(x.dtype)


def evaluate_panorama(render, gt_hdr, gt_depth=None, gt_normal=None, gt_albedo=None, depth_mask=None):
    """Score one rendered panorama.  `render` is render_image's 9-tuple as it is (its [1, C, H, W] views are read in
    place); the ground truths are [1, C, H, W] or [C, H, W] images of the same H x W.  Returns a dict of floats:

    * mse, rmse, l1, psnr, ws_mse, ws_rmse, ws_l1, ws_psnr: fine_rgb against gt_hdr, both HDR (no tone mapping);
    * ldr_psnr, ldr_ws_psnr, ssim, ws_ssim: the validation step's LDR pair (systems/panonerf_system.py:83,92),
      hdr_to_ldr(fine_rgb, dtype='uint8') against hdr_to_ldr(gt_hdr); ws_ssim is ours (see calc_ws_ssim);
    * normal_mae, normal_ws_mae (degrees), normal_cossimi, normal_ws_cossimi: fine_nor against gt_normal put through
      F.normalize twice over the channels (systems/panonerf_system.py:85,96), when gt_normal is given;
    * depth_abs_rel, depth_sq_rel, depth_lin_rms, depth_log_rms, depth_delta1..3: fine_dep against gt_depth over
      depth_mask > 0 (every pixel if depth_mask is None), when gt_depth is given (NaN for an empty selection);
    * albedo_simse, albedo_psnr: the rendered albedo against gt_albedo, both raw, when both exist.

    On CUDA tensors this is a few kernel launches per group and one device-to-host copy of the fp64 sums; otherwise
    the host restatements compute the same sums."""
    _, hdr, _, depth, normal, albedo = render[:6]
    c, h, w = _chw(hdr).shape
    groups = [("hdr", lambda **k: _image_sums(hdr, gt_hdr, **k), _N_SUMS),
              ("ldr", lambda **k: _image_sums(hdr, gt_hdr, TONE_LDR_U8, TONE_LDR, **k), _N_SUMS),
              ("ssim", lambda **k: _ssim_sums(hdr, gt_hdr, TONE_LDR_U8, TONE_LDR, **k)[0], _N_SSIM)]
    if gt_normal is not None:
        groups.append(("normal", lambda **k: _normal_sums(normal, gt_normal, 2, **k), _N_NORMALS))
    if gt_depth is not None:
        groups.append(("depth", lambda **k: _depth_sums(depth, gt_depth, depth_mask, **k), _N_DEPTH))
    if albedo is not None and gt_albedo is not None:
        groups.append(("albedo", lambda **k: _image_sums(albedo, gt_albedo, **k), _N_SUMS))
    sums = {}
    if hdr.is_cuda:
        out = torch.empty(sum(n for *_, n in groups), dtype=torch.float64, device=hdr.device)
        work = _workspace(hdr.device, 3, h, w)
        at = 0
        for name, fn, n in groups:
            fn(out=out[at:at + n], work=work)
            at += n
        flat, at = out.cpu(), 0
        for name, _, n in groups:
            sums[name], at = flat[at:at + n], at + n
    else:
        for name, fn, n in groups:
            sums[name] = fn()
    s, l, v = sums["hdr"], sums["ldr"], sums["ssim"]
    res = {"mse": _mse(s), "rmse": torch.sqrt(_mse(s)), "l1": s[1] / s[5], "psnr": _psnr(s), "ws_mse": s[2],
           "ws_rmse": torch.sqrt(s[2]), "ws_l1": s[3], "ws_psnr": _ws_psnr(s),
           "ldr_psnr": _psnr(l), "ldr_ws_psnr": _ws_psnr(l), "ssim": v[0] / v[2], "ws_ssim": v[1] / c}
    if "normal" in sums:
        n = sums["normal"]
        res.update(normal_mae=n[0] / n[4], normal_ws_mae=n[1], normal_cossimi=n[2] / n[4], normal_ws_cossimi=n[3])
    if "depth" in sums:
        d = sums["depth"]
        res.update(depth_abs_rel=_depth_metric(d, "abs_rel"), depth_sq_rel=_depth_metric(d, "sq_rel"),
                   depth_lin_rms=_depth_metric(d, "lin_rms"), depth_log_rms=_depth_metric(d, "log_rms"),
                   **{f"depth_delta{k}": _depth_metric(d, "delta", k) for k in _DELTA_DEGREES})
    if "albedo" in sums:
        res.update(albedo_simse=_simse(sums["albedo"]), albedo_psnr=_psnr(sums["albedo"]))
    return {k: float(x) for k, x in res.items()}
