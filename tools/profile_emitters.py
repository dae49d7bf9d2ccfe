"""GPU cost of emitter extraction (pano_nerf_amd.emitters).  Three parts, one JSON line:

1. extract_emitters at 64 x 128 for 1 and 64 probes on a seeded PanoMipNeRF (default mode, 128 + 128 samples), split into
   the render (probe_rgbd) and the three steps (emitter_threshold, label_emitters, emitter_stats, each as the module calls
   it: the cumsum, the sort and the host synchronisation included) and their share of the render of the same run.  The
   random model's probes are smooth, so the steps are timed on the rendered probes with two analytic lamps painted in.
2. label_emitters + emitter_stats on one 512 x 1024 panorama: a few-lamp mask and a 0.4-density random mask (tens of
   thousands of components): does the cost of the records depend on the number of components?
3. every entry point alone (the kernels without torch's cumsum / sort), as the mean of --window back-to-back calls between
   two device events, next to the time an HBM copy of the bytes it touches takes at the copy rate measured in the same
   run (a 256 MiB device-to-device copy, read + written bytes).  Bytes per pixel, counted from the code: threshold 16 (the
   three channels and omega); labels 32 (12 radiance, parent written once and read at least twice, roots and flags
   written); compact 12; stats 60 per EMITTER pixel (order twice, radiance, omega, directions twice, distance) - the
   union's chain walks are extra reads of parent that depend on the mask and are not counted.

Per configuration the median of --iters synchronised calls (host clock around a device synchronise, as
tools/profile_objects.py).

    python tools/profile_emitters.py
    python tools/profile_emitters.py --kernels     # no model: parts 2 and 3 only
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pano_nerf_amd import _lib, emitters as em, lighting  # noqa: E402
from tools.profile_objects import setup, timed  # noqa: E402
from tools.profile_textures import windowed  # noqa: E402


def paint_lamps(probes):
    """two discs of radiance 50 and 20 (angular radius 0.35 and 0.3, the first across the seam) painted into [P, 3, H, W]"""
    P, _, H, W = probes.shape
    dirs, _ = lighting.probe_directions(H, W, probes.device)
    out = probes.clone()
    for axis, radius, radiance in (((0.05, 0.3, 1.0), 0.35, 50.0), ((-1.0, -0.4, 0.2), 0.3, 20.0)):
        a = torch.tensor(axis, device=probes.device)
        inside = (torch.acos((dirs @ (a / a.norm())).clamp(-1, 1)) < radius).view(1, 1, H, W)
        out = torch.where(inside, torch.full_like(out, radiance), out)
    return out


def raw_calls(probes, threshold, dist):
    """name -> (callable launching that entry point alone on prepared buffers, bytes it touches)"""
    x, sp, sc, sw, P, H, W = lighting._probe_view(probes)
    dev, HW = x.device, H * W
    dirs, omega = lighting.probe_directions(H, W, dev)
    st = _lib.stream(dev)
    thr = torch.empty(P, device=dev)
    parent, flags = (torch.empty(P, HW, dtype=torch.int32, device=dev) for _ in range(2))
    roots = torch.empty(P, H, W, dtype=torch.int32, device=dev)
    count = torch.empty(P, dtype=torch.int32, device=dev)
    labels, cnt = em.label_emitters(probes, threshold)
    C = int(cnt.max())
    S = P * C
    lab = labels.view(P, HW).to(torch.int64)
    key = torch.where(lab >= 0, lab + torch.arange(P, device=dev).view(P, 1) * C, S).view(-1)
    skey, order = torch.sort(key, stable=True)
    starts = torch.searchsorted(skey, torch.arange(S + 1, dtype=torch.int64, device=dev))
    outs = em.emitter_stats(probes, labels, cnt, dist)
    z = dist.contiguous()
    _lib.call("pn_emitter_labels", P, H, W, x.data_ptr(), sp, sc, sw, threshold.data_ptr(), parent.data_ptr(),
              roots.data_ptr(), flags.data_ptr(), st)
    prefix = torch.cumsum(flags, 1, dtype=torch.int32)
    scratch = roots.clone()
    emitters = int((labels >= 0).sum())
    calls = {
        "threshold": (lambda: _lib.call("pn_emitter_threshold", P, H, W, x.data_ptr(), sp, sc, sw, omega.data_ptr(), 8.0,
                                        thr.data_ptr(), st), 16 * P * HW),
        "labels": (lambda: _lib.call("pn_emitter_labels", P, H, W, x.data_ptr(), sp, sc, sw, threshold.data_ptr(),
                                     parent.data_ptr(), roots.data_ptr(), flags.data_ptr(), st), 32 * P * HW),
        # compact works in place: it is timed on a scratch copy that holds roots the first time and labels after (the
        # same loads and stores either way)
        "compact": (lambda: _lib.call("pn_emitter_compact", P, H, W, prefix.data_ptr(), scratch.data_ptr(), count.data_ptr(),
                                      st), 12 * P * HW),
        "stats": (lambda: _lib.call("pn_emitter_stats", P, H, W, x.data_ptr(), sp, sc, sw, dirs.data_ptr(), omega.data_ptr(),
                                    z.data_ptr(), C, P * HW, order.data_ptr(), starts.data_ptr(),
                                    *(outs[k].data_ptr() for k in em._FIELDS), st), 60 * emitters + 56 * S),
    }
    return calls, dict(components_max=C, components=int(cnt.sum()), emitter_pixels=emitters)


def steps(probes, dist, iters, out, tag):
    """the three steps as the module runs them, synchronised medians in ms"""
    out[f"{tag}_threshold_ms"], thr = timed(lambda: em.emitter_threshold(probes), iters)
    out[f"{tag}_labels_ms"], (labels, count) = timed(lambda: em.label_emitters(probes, thr), iters)
    out[f"{tag}_stats_ms"], _ = timed(lambda: em.emitter_stats(probes, labels, count, dist), iters)
    out[f"{tag}_components"] = int(count.sum())
    return thr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--kernels", action="store_true", help="no model: the 512 x 1024 panorama and the entry points only")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    out = dict(iters=a.iters, window=a.window)
    src = torch.empty(1 << 26, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    ms = windowed(lambda: dst.copy_(src), 20)
    rate = 2 * src.numel() * 4 / (1e-3 * ms)
    out["hbm_copy_GBps"] = rate / 1e9
    del src, dst
    rng = np.random.default_rng(0)
    # 1. extract_emitters end to end
    if not a.kernels:
        model = setup()
        for P in (1, 64):
            pos = torch.from_numpy((0.4 * (rng.random((P, 3)) - 0.5)).astype(np.float32)).to(dev)
            tag = f"extract_64x128_P{P}"
            out[f"{tag}_render_ms"], (probes, dist) = timed(lambda: em.probe_rgbd(model, pos, 64, 128), a.iters)
            out[f"{tag}_all_ms"], _ = timed(lambda: em.extract_emitters(model, pos, (64, 128)), a.iters)
            lamps = paint_lamps(probes)
            steps(lamps, dist, a.iters, out, tag)
            out[f"{tag}_from_probes_ms"], lists = timed(lambda: em.emitters_from_probes(lamps, pos, dist), a.iters)
            out[f"{tag}_emitters_found"] = sum(len(x) for x in lists)
            three = sum(out[f"{tag}_{k}_ms"] for k in ("threshold", "labels", "stats"))
            out[f"{tag}_three_steps_share_of_render"] = three / out[f"{tag}_render_ms"]
            out[f"{tag}_from_probes_share_of_render"] = out[f"{tag}_from_probes_ms"] / out[f"{tag}_render_ms"]
    # 2. one 512 x 1024 panorama: a few lamps, and a 0.4-density random mask
    H, W = 512, 1024
    base = torch.from_numpy((0.2 * rng.random((1, 3, H, W))).astype(np.float32)).to(dev)
    dist = torch.from_numpy((1.0 + 3.0 * rng.random((1, H, W))).astype(np.float32)).to(dev)
    noisy = torch.where(torch.from_numpy(rng.random((1, 1, H, W)) < 0.4).to(dev), base + 30.0, base)
    for tag, probes in (("pano_512x1024_lamps", paint_lamps(base)), ("pano_512x1024_random_0.4", noisy)):
        thr = torch.full((1,), 5.0, device=dev)
        out[f"{tag}_labels_ms"], (labels, count) = timed(lambda: em.label_emitters(probes, thr), a.iters)
        out[f"{tag}_stats_ms"], _ = timed(lambda: em.emitter_stats(probes, labels, count, dist), a.iters)
        # 3. the entry points alone, next to a copy of their bytes
        calls, info = raw_calls(probes, thr, dist)
        out.update({f"{tag}_{k}": v for k, v in info.items()})
        for name, (fn, nbytes) in calls.items():
            t = windowed(fn, a.window)
            out[f"{tag}_{name}_kernel_ms"] = t
            out[f"{tag}_{name}_bytes"] = nbytes
            out[f"{tag}_{name}_copy_of_bytes_ms"] = 1e3 * nbytes / rate
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
