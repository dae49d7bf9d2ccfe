"""The evaluation metrics added next to metrics.py's calc_* family (SSIM, depth, calc_simse, normal sums, tone-mapped
pairs, evaluate_panorama) against values captured from the reference (tests/golden/metrics_ext.npz, made by
tests/golden/make_metrics_ext_golden.py).  Here on the host restatements; test_gpu_metrics.py runs the same checks on
the HIP kernels.  Also the status codes of the new C entry points (host-side checks only, no launch)."""
import math

import numpy as np
import pytest
import torch

from pano_nerf_amd import _lib, metrics

SIZES = ((5, 9), (8, 16), (16, 32), (37, 70))
SCALAR_RTOL = 1e-5
MAP_ATOL = 1e-5
LDR_MAP_ATOL = 1e-4


def close(got, want, name, rtol=SCALAR_RTOL):
    got, want = float(got), float(want)
    if math.isnan(want):
        assert math.isnan(got), (name, got, want)
    elif math.isinf(want):
        assert got == want, (name, got, want)
    else:
        assert abs(got - want) <= rtol * max(abs(want), 1e-2), (name, got, want)


def check_golden(g, h, w, dev):
    """Every new function on tensors placed on `dev` against the reference's outputs at size h x w."""
    k = f"{h}x{w}/"
    T = lambda name: torch.tensor(g[k + name]).to(dev)
    pred, gt = T("pred"), T("gt")
    # tone mapping inside the kernels: no element of hdr_to_ldr(pred, 'uint8') / hdr_to_ldr(gt) differs from the
    # reference's by more than rounding (a uint8 truncation that went the other way would add >= 1e-6 here)
    for tone, ref in ((metrics.TONE_LDR_U8, pred), (metrics.TONE_LDR, gt)):
        s = metrics._image_sums(ref, T("ldr_pred" if ref is pred else "ldr_gt"), tone).cpu()
        assert float(s[0]) < 1e-9, (k, tone, float(s[0]))
    # the SSIM map of the validation pair, element-wise, against the reference run on fp64 copies of its LDR images.
    # The saturated, quantised pair has near-flat windows where (E[x^2] - mu^2) cancels: there the reference's fp32 map
    # carries up to ~1e-4 of noise, and a one-ulp difference of pow() between two math libraries moves the map by
    # ~1e-5, hence the wider bound on this map (the plain pair below is held to MAP_ATOL)
    smap = metrics._ssim_sums(pred[0], gt[0], metrics.TONE_LDR_U8, metrics.TONE_LDR, want_map=True)[1]
    assert np.abs(smap.cpu().numpy() - g[k + "ssim_ldr_map64"][0]).max() <= LDR_MAP_ATOL, k
    assert np.abs(smap.cpu().numpy() - g[k + "ssim_ldr_map"][0]).max() <= 2 * LDR_MAP_ATOL, k
    ldr_map = metrics.ssim(T("ldr_pred"), T("ldr_gt")).cpu().numpy()
    assert np.abs(ldr_map - g[k + "ssim_ldr_map64"]).max() <= LDR_MAP_ATOL, k
    # SSIM on a plain pair: every reduction, max_val, one channel
    a, b = T("ssim_a"), T("ssim_b")
    close(metrics.calc_ssim(a, b), g[k + "ssim_mean"], k + "ssim_mean")
    close(metrics.ssim(a, b, reduction="sum"), g[k + "ssim_sum"], k + "ssim_sum")
    close(metrics.ssim(a, b, reduction="mean", max_val=2.0), g[k + "ssim_mean_max2"], k + "ssim_mean_max2")
    m = metrics.ssim(a, b, reduction="none")
    assert m.shape == a.shape and m.dtype == torch.float32
    assert np.abs(m.cpu().numpy() - g[k + "ssim_map"]).max() <= MAP_ATOL, k
    m1 = metrics.ssim(a[:, :1], b[:, :1], window_size=11, reduction="none")
    assert np.abs(m1.cpu().numpy() - g[k + "ssim_c1_map"]).max() <= MAP_ATOL, k
    # depth, with a mask that has zeros and with an all-zero mask (NaN)
    dp, dg, mask = T("depth_pred"), T("depth_gt"), T("depth_mask")
    for tag, msk in (("", mask), ("empty_", torch.zeros_like(mask))):
        close(metrics.abs_rel_error(dp, dg, msk), g[k + tag + "abs_rel"], k + tag + "abs_rel")
        close(metrics.sq_rel_error(dp, dg, msk), g[k + tag + "sq_rel"], k + tag + "sq_rel")
        close(metrics.lin_rms_sq_error(dp, dg, msk), g[k + tag + "lin_rms"], k + tag + "lin_rms")
        close(metrics.log_rms_sq_error(dp, dg, msk), g[k + tag + "log_rms"], k + tag + "log_rms")
        for deg in (1, 2, 3):
            close(metrics.delta_inlier_ratio(dp, dg, msk, degree=deg), g[k + tag + f"delta{deg}"], k + tag + f"d{deg}")
    # albedo
    close(metrics.calc_simse(T("albedo"), T("albedo_gt")), g[k + "simse"], k + "simse")
    # normals with identical, antiparallel, scaled and zero vectors mixed in
    s = metrics._normal_sums(T("n1"), T("n2")).cpu()
    close(s[0] / s[4], g[k + "mae"], k + "mae")
    close(s[1], g[k + "ws_mae"], k + "ws_mae")
    close(s[2] / s[4], g[k + "cossimi"], k + "cossimi")
    close(s[3], g[k + "ws_cossimi"], k + "ws_cossimi")
    # evaluate_panorama on the same images (HDR, LDR, depth and albedo keys)
    render = (None, pred, None, dp, None, T("albedo"), None, None, None)
    res = metrics.evaluate_panorama(render, gt, gt_depth=dg, gt_albedo=T("albedo_gt"), depth_mask=mask)
    for key in ("mse", "rmse", "l1", "psnr", "ws_mse", "ws_rmse", "ws_l1", "ws_psnr", "ldr_psnr", "ldr_ws_psnr"):
        close(res[key], g[k + key], k + key)
    close(res["ssim"], g[k + "calc_ssim_ldr"], k + "ssim")
    for key in ("abs_rel", "sq_rel", "lin_rms", "log_rms", "delta1", "delta2", "delta3"):
        close(res["depth_" + key], g[k + key], k + key)
    close(res["albedo_simse"], g[k + "simse"], k + "albedo_simse")
    return res


@pytest.mark.parametrize("h,w", SIZES)
def test_host_metrics_match_reference(golden, h, w):
    g = golden("metrics_ext")
    k = f"{h}x{w}/"
    ldr = metrics._tonemap(torch.tensor(g[k + "pred"]), metrics.TONE_LDR_U8)
    assert np.abs(ldr.numpy() - g[k + "ldr_pred"]).max() <= 1e-6
    assert np.array_equal(metrics._tonemap(torch.tensor(g[k + "gt"]), metrics.TONE_LDR).numpy() > 0, g[k + "ldr_gt"] > 0)
    res = check_golden(g, h, w, "cpu")
    assert set(res) == {"mse", "rmse", "l1", "psnr", "ws_mse", "ws_rmse", "ws_l1", "ws_psnr", "ldr_psnr", "ldr_ws_psnr",
                        "ssim", "ws_ssim", "depth_abs_rel", "depth_sq_rel", "depth_lin_rms", "depth_log_rms",
                        "depth_delta1", "depth_delta2", "depth_delta3", "albedo_simse", "albedo_psnr"}


def test_ws_ssim_is_the_solid_angle_weighted_map(golden):
    g = golden("metrics_ext")
    for h, w in SIZES:
        a, b = torch.tensor(g[f"{h}x{w}/ssim_a"]), torch.tensor(g[f"{h}x{w}/ssim_b"])
        sa = metrics.solid_angle_refinement(h, w).double().reshape(1, 1, h, w)
        want = (torch.tensor(g[f"{h}x{w}/ssim_map"]).double() * sa / sa.sum()).sum() / 3
        assert abs(float(metrics.calc_ws_ssim(a, b)) - float(want)) < 1e-6
        assert abs(float(metrics.calc_ws_ssim(a[0], b[0])) - float(want)) < 1e-6


def test_normals_follow_cosine_similarity_edge_cases():
    """torch's F.cosine_similarity on fp32: a zero vector gives cos 0 (90 degrees); a cosine that rounds past +-1 gives
    a NaN angle that nan_to_num makes 0 degrees, so identical and antiparallel pairs may both score 0."""
    x = torch.tensor([[0.0, 0.0, 2.0], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [0.3, -0.7, 0.2], [0.3, -0.7, 0.2]])
    y = torch.tensor([[0.0, 0.0, -3.0], [1.0, 2.0, 3.0], [1.0, 0.0, 0.0], [0.3, -0.7, 0.2], [-0.3, 0.7, -0.2]])
    cos = torch.nn.functional.cosine_similarity(x, y, dim=-1)
    ang = torch.nan_to_num(torch.acos(cos.double()) * (180 / math.pi), nan=0.0)
    s = metrics._normal_sums(x.T.reshape(3, 1, 5), y.T.reshape(3, 1, 5))
    assert float(ang[0]) == 180.0 and float(ang[2]) == 90.0
    assert float(s[0]) == pytest.approx(float(ang.sum()), rel=1e-12)
    assert float(s[2]) == pytest.approx(float(cos.double().sum()), rel=1e-12)


def test_metric_entry_points_reject_bad_arguments():
    """Host-side checks of the new C ABI, before any launch (no GPU needed)."""
    lib = _lib.load()
    assert lib.pn_metrics_work_doubles(3, 512, 1024) >= 3 * 32 * 32 * 3
    assert lib.pn_metrics_work_doubles(3, 1, 1) > 0
    for c, h, w in ((2, 8, 8), (3, 0, 8), (3, 8, 0), (1, -1, 4)):
        assert lib.pn_metrics_work_doubles(c, h, w) == -1
        assert lib.pn_metric_sums(c, h, w, 1, 1, 3, 0, 1, 1, 3, 0, 1, 1, None) == -1
        assert lib.pn_metric_ssim(c, h, w, 1, 1, 3, 0, 1, 1, 3, 0, 11, 1, 1.0, None, 1, 1, None) == -1
    assert lib.pn_metric_sums(3, 8, 8, 1, 1, 3, 3, 1, 1, 3, 0, 1, 1, None) == -2  # unknown tone mode
    assert lib.pn_metric_ssim(3, 8, 8, 1, 1, 3, 0, 1, 1, 3, -1, 11, 1, 1.0, None, 1, 1, None) == -2
    assert lib.pn_metric_ssim(3, 8, 8, 1, 1, 3, 0, 1, 1, 3, 0, 7, 1, 1.0, None, 1, 1, None) == -2  # window 11 only
    assert lib.pn_metric_ssim(3, 8, 8, 1, 1, 3, 0, 1, 1, 3, 0, 11, None, 1.0, None, 1, 1, None) == -3  # no taps
    assert lib.pn_metric_normals(0, 8, 1, 1, 3, 1, 1, 3, 0, 1, 1, None) == -1
    assert lib.pn_metric_normals(8, 8, 1, 1, 3, 1, 1, 3, 3, 1, 1, None) == -2
    assert lib.pn_metric_depth(0, 1, 1, 1, 1, None, 0, 1, 1, None) == -1
    assert lib.pn_metric_depth(8, None, 1, 1, 1, None, 0, 1, 1, None) == -3
