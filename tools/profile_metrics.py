"""GPU cost of scoring one 512 x 1024 panorama: metrics.evaluate_panorama (the pn_metrics.hip kernels) next to the same
metric set written as torch ops on the device (fp32, the reference's formulation: conv2d SSIM, masked depth selections,
one host copy at the end).  One leg per process so that a kernel trace holds one leg only:

    python tools/profile_metrics.py --leg kernels|torch [--iters 50]          # wall time per call (synchronised)
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/profile_metrics.py --leg kernels --iters 20
"""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pano_nerf_amd import metrics  # noqa: E402


def panorama(h, w, seed=5):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    rgb = torch.rand(h * w, 3, generator=gen) * 2.5
    depth = torch.rand(h * w, 1, generator=gen) * 5 + 0.2
    normal = torch.randn(h * w, 3, generator=gen)
    albedo = torch.rand(h * w, 3, generator=gen)
    view = lambda x: x.cuda().view(1, h, w, -1).permute(0, 3, 1, 2)
    chw = lambda x: x.view(1, h, w, -1).permute(0, 3, 1, 2).contiguous().cuda()
    render = (None, view(rgb), None, view(depth), view(normal), view(albedo), None, None, None)
    gt = dict(gt_hdr=chw(rgb * 1.1), gt_depth=chw(depth * 0.9), gt_normal=chw(normal + 0.3),
              gt_albedo=chw(albedo * 0.95), depth_mask=chw((torch.rand(h * w, 1, generator=gen) > 0.3).float()))
    return render, gt


def torch_ops(render, gt_hdr, gt_depth, gt_normal, gt_albedo, depth_mask):
    """The same keys as evaluate_panorama with fp32 torch ops on the device and one device-to-host copy."""
    pred, dep, nor, alb = render[1][0], render[3], render[4], render[5]
    gt = gt_hdr[0]
    c, h, w = pred.shape
    wt = metrics.solid_angle_refinement(h, w, device=pred.device).reshape(1, h, w)
    wt = wt / wt.sum()
    d = pred - gt
    out = [torch.mean(d ** 2), torch.mean(d ** 2) ** 0.5, d.abs().mean(), -10 * torch.log10(torch.mean(d ** 2)),
           torch.sum(d ** 2 * wt), torch.sqrt(torch.sum(d ** 2 * wt)), torch.sum(d.abs() * wt),
           -10 * torch.log10(torch.sum(d ** 2 * wt))]
    lp, lg = metrics._tonemap(pred, metrics.TONE_LDR_U8), metrics._tonemap(gt, metrics.TONE_LDR)
    dl = lp - lg
    out += [-10 * torch.log10(torch.mean(dl ** 2)), -10 * torch.log10(torch.sum(dl ** 2 * wt))]
    g = metrics._gaussian_taps(11).to(pred.device)
    win = (g[:, None] * g[None, :]).expand(c, 1, 11, 11)
    blur = lambda v: F.conv2d(v[None], win, padding=5, groups=c)[0]
    m1, m2 = blur(lp), blur(lg)
    s11, s22, s12 = blur(lp * lp) - m1 * m1, blur(lg * lg) - m2 * m2, blur(lp * lg) - m1 * m2
    smap = ((2 * m1 * m2 + 1e-4) * (2 * s12 + 9e-4)) / ((m1 * m1 + m2 * m2 + 1e-4) * (s11 + s22 + 9e-4))
    out += [smap.mean(), (smap * wt).sum() / c]
    gn = F.normalize(F.normalize(gt_normal, dim=1), dim=1)
    cos = F.cosine_similarity(nor, gn, dim=1)
    ang = torch.nan_to_num(torch.acos(cos) / math.pi * 180, nan=0.0)
    out += [ang.mean(), (ang * wt).sum(), cos.mean(), (cos * wt).sum()]
    sel = depth_mask > 0
    p, q = dep[sel], gt_depth[sel]
    lsel = sel & (dep > 1e-7) & (gt_depth > 1e-7)
    r = torch.max(p / q, q / p)
    out += [((p - q).abs() / q).mean(), ((p - q) ** 2 / q).mean(), torch.sqrt(((p - q) ** 2).mean()),
            torch.sqrt(((dep[lsel].log() - gt_depth[lsel].log()) ** 2).mean())]
    out += [(r < 1.25 ** k).float().mean() for k in (1, 2, 3)]
    da = alb - gt_albedo
    out += [torch.var(da), -10 * torch.log10(torch.mean(da ** 2))]
    return torch.stack(out).cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("kernels", "torch"), required=True)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--h", type=int, default=512)
    ap.add_argument("--w", type=int, default=1024)
    a = ap.parse_args()
    render, gt = panorama(a.h, a.w)
    fn = (lambda: metrics.evaluate_panorama(render, **gt)) if a.leg == "kernels" else (lambda: torch_ops(render, **gt))
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.iters
    print(json.dumps({"leg": a.leg, "h": a.h, "w": a.w, "iters": a.iters, "wall_ms_per_call": round(ms, 4)}))


if __name__ == "__main__":
    main()
