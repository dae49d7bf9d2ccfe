"""Golden vectors for the evaluation metrics added after metrics.npz (SSIM, depth, calc_simse, normals with edge cases,
tone-mapped pairs) by IMPORTING the reference's utils/metrics.py and hdr_to_ldr.

Build container only (needs a checkout of the reference at REF); stores seeded inputs and the reference's outputs, no
reference code.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_metrics_ext_golden.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
for name in ("cv2", "Imath"):
    sys.modules[name] = types.ModuleType(name)
_exr = types.ModuleType("OpenEXR")
_exr.InputFile = _exr.OutputFile = _exr.Header = object
sys.modules["OpenEXR"] = _exr

import numpy as np  # noqa: E402
import torch  # noqa: E402

import utils.metrics as rm  # noqa: E402
from utils.surface_rendering import hdr_to_ldr  # noqa: E402

SIZES = ((5, 9), (8, 16), (16, 32), (37, 70))  # 5 x 9: H < 11, smaller than the SSIM window; 37 x 70 divides no tile
rng = np.random.Generator(np.random.PCG64(23))
t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))
out = {}
for h, w in SIZES:
    k = f"{h}x{w}/"
    # HDR pair: mostly in [0, 3), some pixels past the ACES knee (~7.2, where hdr_to_ldr clamps) and some negative
    pred = rng.random((1, 3, h, w)) * 3
    gt = np.clip(pred + 0.4 * rng.standard_normal((1, 3, h, w)), -0.5, None)
    for a in (pred, gt):
        a[rng.random(a.shape) < 0.08] *= 6.0
        a[rng.random(a.shape) < 0.05] *= -0.2
    pred, gt = t(pred), t(gt)
    out[k + "pred"], out[k + "gt"] = pred, gt
    ldr_pred, ldr_gt = hdr_to_ldr(pred, dtype="uint8"), hdr_to_ldr(gt)
    out[k + "ldr_pred"], out[k + "ldr_gt"] = ldr_pred, ldr_gt
    for name, fn in (("mse", rm.calc_mse), ("rmse", rm.calc_rmse), ("l1", rm.calc_l1), ("psnr", rm.calc_psnr)):
        out[k + name] = fn(pred, gt)
    for name, fn in (("ws_mse", rm.calc_ws_mse), ("ws_rmse", rm.calc_ws_rmse), ("ws_l1", rm.calc_ws_l1),
                     ("ws_psnr", rm.calc_ws_psnr)):
        out[k + name] = fn(pred[0], gt[0])
    out[k + "ldr_psnr"] = rm.calc_psnr(ldr_pred, ldr_gt)
    out[k + "ldr_ws_psnr"] = rm.calc_ws_psnr(ldr_pred[0], ldr_gt[0])
    # SSIM: a plain [0, 1] pair (also with max_val 2 and one channel) and the tone-mapped pair
    a, b = t(rng.random((1, 3, h, w))), t(rng.random((1, 3, h, w)))
    b = 0.6 * a + 0.4 * b
    out[k + "ssim_a"], out[k + "ssim_b"] = a, b
    out[k + "ssim_mean"] = rm.ssim(a, b, window_size=11, reduction="mean")
    out[k + "ssim_sum"] = rm.ssim(a, b, window_size=11, reduction="sum")
    out[k + "ssim_map"] = rm.ssim(a, b, window_size=11, reduction="none")
    out[k + "ssim_mean_max2"] = rm.ssim(a, b, window_size=11, reduction="mean", max_val=2.0)
    out[k + "ssim_c1_map"] = rm.ssim(a[:, :1], b[:, :1], window_size=11, reduction="none")
    out[k + "calc_ssim_ldr"] = rm.calc_ssim(ldr_pred, ldr_gt)
    out[k + "ssim_ldr_map"] = rm.ssim(ldr_pred, ldr_gt, window_size=11, reduction="none")
    # the same on fp64 copies: the saturated, quantised LDR pair has near-flat windows where the fp32 map carries
    # ~1e-4 of cancellation noise (E[x^2] - mu^2)
    out[k + "ssim_ldr_map64"] = rm.ssim(ldr_pred.double(), ldr_gt.double(), window_size=11, reduction="none").float()
    # depth: positive depths with zeros, values at and below 1e-7, and a mask with zeros; an all-zero mask
    dp = rng.random((1, 1, h, w)) * 4 + 0.5
    dg = dp * np.exp(0.3 * rng.standard_normal((1, 1, h, w)))
    mask = rng.random((1, 1, h, w)) > 0.25
    for a in (dp, dg):
        flat = a.reshape(-1)
        pick = rng.choice(flat.size, size=max(3, flat.size // 12), replace=False)
        flat[pick[0::3]] = 0.0
        flat[pick[1::3]] = 1e-8
        flat[pick[2::3]] = np.float32(1e-7)
    if h != 5:  # a zero gt depth under the mask makes abs_rel / sq_rel inf: kept for the smallest size only
        mask.reshape(-1)[dg.reshape(-1) == 0] = False
    dp, dg, mask = t(dp), t(dg), t(mask)
    out[k + "depth_pred"], out[k + "depth_gt"], out[k + "depth_mask"] = dp, dg, mask
    zero = torch.zeros_like(mask)
    for tag, m in (("", mask), ("empty_", zero)):
        out[k + tag + "abs_rel"] = rm.abs_rel_error(dp, dg, m)
        out[k + tag + "sq_rel"] = rm.sq_rel_error(dp, dg, m)
        out[k + tag + "lin_rms"] = rm.lin_rms_sq_error(dp, dg, m)
        out[k + tag + "log_rms"] = rm.log_rms_sq_error(dp, dg, m)
        for deg in (1, 2, 3):
            out[k + tag + f"delta{deg}"] = rm.delta_inlier_ratio(dp, dg, m, degree=deg)
    # albedo
    alb, alb_gt = t(rng.random((1, 3, h, w))), t(rng.random((1, 3, h, w)))
    out[k + "albedo"], out[k + "albedo_gt"] = alb, alb_gt
    out[k + "simse"] = rm.calc_simse(alb, alb_gt)
    # normals [1, 3, H, W] with identical, antiparallel, scaled-identical and zero vectors mixed in
    n1 = rng.standard_normal((h * w, 3))
    n2 = n1 + 0.3 * rng.standard_normal((h * w, 3))
    kind = rng.integers(0, 6, size=h * w)
    n2[kind == 1] = n1[kind == 1]
    n2[kind == 2] = -n1[kind == 2]
    n2[kind == 3] = 2.5 * n1[kind == 3]
    n1[kind == 4] = 0.0
    n2[kind == 5] = 0.0
    n1, n2 = t(n1.T.reshape(1, 3, h, w)), t(n2.T.reshape(1, 3, h, w))
    out[k + "n1"], out[k + "n2"] = n1, n2
    out[k + "mae"] = rm.calc_mae(n1, n2, dim=1)
    out[k + "ws_mae"] = rm.calc_ws_mae(n1, n2, dim=1)
    out[k + "cossimi"] = rm.calc_cossimi(n1, n2, dim=1)
    out[k + "ws_cossimi"] = rm.calc_ws_cossimi(n1[0], n2[0], dim=0)
np.savez_compressed(os.path.join(HERE, "metrics_ext.npz"), **{k: np.asarray(v) for k, v in out.items()})
print(len(out), "arrays;", os.path.getsize(os.path.join(HERE, "metrics_ext.npz")), "bytes")
