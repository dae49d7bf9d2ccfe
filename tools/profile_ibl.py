"""GPU cost of baking light probes into image-based lighting (pano_nerf_amd.ibl) on seeded random probes: bake_ibl for one
and for 64 probes of 32 x 64 at size 32 and for one probe of 256 x 512 at size 64, stage by stage (level 0 =
probes_to_cubemaps, every filtered level, the irradiance cube, the table) with each stage's share of the sum; prefilter
in (direction, pixel) pairs per second next to lighting.irradiance over the same pairs; brdf_lut(32, 256); ibl_shade of
480 x 640 rows next to objects.shade (microfacet) on the same rows under a 32 x 64 probe.  Every time is the mean of a
window of back-to-back calls between two device events after a warm-up call (tools/profile_textures.py's windowed); the
HBM copy rate of the run (a 1 GiB device-to-device copy, read + written bytes) is there for scale.  One JSON line.

    python tools/profile_ibl.py
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pano_nerf_amd import ibl, lighting, objects  # noqa: E402
from tools.profile_textures import windowed  # noqa: E402


def probes_of(P, H, W, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(P, H, W, 3, generator=g) * 2.0 + 0.05
    x[torch.rand(P, H, W, generator=g) < 0.01] *= 20.0
    return x.to(dev).permute(0, 3, 1, 2)  # the view light_probes returns


def unit(n, dev, seed):
    v = torch.randn(n, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (v / v.norm(dim=-1, keepdim=True)).to(torch.float32).to(dev)


def bake_stages(probes, size, window):
    """ms per stage of bake_ibl(probes, size) and of the whole call"""
    dev = probes.device
    levels = size.bit_length() - 2
    out = {"bake_ibl_ms": windowed(lambda: ibl.bake_ibl(probes, size), window),
           "level0_probes_to_cubemaps_ms": windowed(lambda: lighting.probes_to_cubemaps(probes, size, 4), window)}
    for l in range(1, levels):
        n = ibl._texel_directions(size >> l, dev)
        r = l / (levels - 1)
        out[f"level{l}_prefilter_{size >> l}_ms"] = windowed(lambda: ibl.prefilter(probes, n, r), window)
    out["irradiance_cube_8_ms"] = windowed(lambda: ibl.irradiance_cubemaps(probes, 8), window)
    out["brdf_lut_32_256_ms"] = windowed(lambda: ibl.brdf_lut(32, 256, dev), window)
    total = sum(v for k, v in out.items() if k != "bake_ibl_ms")
    out["stage_sum_ms"] = total
    out["shares"] = {k[:-3]: round(v / total, 4) for k, v in out.items() if k.endswith("_ms") and k not in ("bake_ibl_ms", "stage_sum_ms")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    out = dict(window=a.window)
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    out["hbm_copy_GBps"] = 2 * src.numel() * 4 / (1e-3 * windowed(lambda: dst.copy_(src), 20)) / 1e9
    del src, dst
    out["bake_1x32x64_size32"] = bake_stages(probes_of(1, 32, 64, dev, 0), 32, a.window)
    out["bake_64x32x64_size32"] = bake_stages(probes_of(64, 32, 64, dev, 1), 32, a.window)
    out["bake_1x256x512_size64"] = bake_stages(probes_of(1, 256, 512, dev, 2), 64, max(2, a.window // 4))
    # prefilter next to irradiance: the same loads, one more division
    for name, (P, H, W, K) in {"64x32x64_K1536": (64, 32, 64, 1536), "1x256x512_K6144": (1, 256, 512, 6144)}.items():
        probes, n = probes_of(P, H, W, dev, 3), unit(K, dev, 4)
        pairs = P * K * H * W
        tp = windowed(lambda: ibl.prefilter(probes, n, 0.5), a.window)
        ti = windowed(lambda: lighting.irradiance(probes, n), a.window)
        out[f"pairs_{name}"] = dict(pairs=pairs, prefilter_ms=tp, irradiance_ms=ti, prefilter_pairs_per_s=pairs / (1e-3 * tp),
                                    irradiance_pairs_per_s=pairs / (1e-3 * ti))
    # the engine's evaluation next to the reference's sum over every probe pixel
    R = 480 * 640
    probes = probes_of(1, 32, 64, dev, 5)
    baked = ibl.bake_ibl(probes, 32)
    albedo, nrm, vd = torch.rand(R, 3, device=dev), unit(R, dev, 6), unit(R, dev, 7)
    rough = torch.rand(R, 1, device=dev)
    out["rows"] = R
    out["ibl_shade_ms"] = windowed(lambda: ibl.ibl_shade(baked, albedo, nrm, vd, rough), a.window)
    out["objects_shade_microfacet_ms"] = windowed(lambda: objects.shade(probes, albedo, nrm, vd, rough), a.window)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
