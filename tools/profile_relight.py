"""GPU cost of relighting (pano_nerf_amd.relight) on a seeded PanoMipNeRF (default mlp_mode, default samples per level),
written as a text report (default profiles/relight.txt):

  relight of one 480 x 640 frame (render_view's fine_rgb, fine_dep, fine_nor, albedo) under 1, 4 and 16 lights at pcf 1 / 3 /
  5 against 64 x 128 panorama maps: ms per call, (row, light) pairs per second, and the bytes the taps gather per second
  (lookups x k^2 x 4 taps x 4 bytes; the lookups are counted by one call against empty maps, where visibility is 1 exactly
  where a lookup was made) next to the HBM copy rate of the run;
  the same frame's render_view (rgb, depth, normal, albedo), in the same run;
  shadow_maps for those lights next to lighting.light_probes of the same size, alternating;
  the kernel's registers and scratch, copied from a compiler report when one is given (--resources FILE, the output of
  hipcc ... -Rpass-analysis=kernel-resource-usage -c pn_relight.hip).

Kernel calls are timed as windows of back-to-back calls between two device events after a warm-up call, --repeats windows
each (min / median / max); the renders by a host clock around a synchronised call, --repeats times.  The model is
random-initialised: its depths and normals are not a room's, so the share of pairs that face their light is what it is
(the report states it).

    python tools/profile_relight.py [--out profiles/relight.txt] [--resources usage.log]
"""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pano_nerf_amd as pn  # noqa: E402
from oracle import pano_oracle as orc  # noqa: E402
from pano_nerf_amd import lighting, relight as rl, views  # noqa: E402
from tools.profile_textures import windowed  # noqa: E402

H, W, HM, WM = 480, 640, 64, 128


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(xs):
    return min(xs), float(np.median(xs)), max(xs)


def make_lights(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        p = rng.uniform(-1.0, 1.0, 3)
        if i % 2:
            out.append(rl.PointLight(p, rng.uniform(1.0, 4.0, 3), axis=rng.normal(size=3), inner_deg=30.0, outer_deg=60.0))
        else:
            out.append(rl.PointLight(p, rng.uniform(1.0, 4.0, 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relight.txt"))
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"Relighting on one MI355X, tools/profile_relight.py --window {a.window} --repeats {a.repeats} (one process, one run).")
    say(f"Kernel calls: mean ms of a window of {a.window} back-to-back calls between two device events after a warm-up call,")
    say(f"{a.repeats} windows each, as min / median / max; whole Python calls.  Renders: host clock around one synchronised call.")
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    hbm = [2 * src.numel() * 4 / (1e-3 * windowed(lambda: dst.copy_(src), 20)) / 1e12 for _ in range(3)]
    del src, dst
    say("HBM copy rate of the run (1 GiB device to device, read + written bytes): %.2f / %.2f / %.2f TB/s." % stats(hbm))
    say()

    model = pn.PanoMipNeRF(rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    model.mlp.load_state_dict(orc.init_params(4, 5))
    model = model.to(dev)
    env = pn.generate_lit_rays(10, 0.01)
    cam = views.perspective_camera(H, W, fov_x_deg=60.0)
    c2w = views.look_at([0.2, 0.1, 1.5], [0.0, 0.0, 0.0])
    outputs = ("rgb", "depth", "normal", "albedo")
    views.render_view(model, views.perspective_camera(48, 64, fov_x_deg=60.0), c2w, env, outputs)  # warm-up
    t_view = [timed(lambda: views.render_view(model, cam, c2w, env, outputs)) for _ in range(a.repeats)]
    view = views.render_view(model, cam, c2w, env, outputs)
    R = H * W
    say(f"render_view of the {H} x {W} frame (rgb, depth, normal, albedo; mlp_mode {model.mlp_mode}, {model.num_samples} samples a level):")
    say("  %.3f / %.3f / %.3f s, %.3g rays/s at the median" % (*stats(t_view), R / stats(t_view)[1]))
    say()

    lights = make_lights(16)
    pos = torch.from_numpy(rl.light_rows(lights)[:, :3].copy()).to(dev)
    say(f"shadow_maps ({HM} x {WM} panorama) next to lighting.light_probes of the same size, alternating, seconds per call:")
    for L in (1, 4, 16):
        ts, tp = [], []
        for _ in range(a.repeats):
            ts.append(timed(lambda: rl.shadow_maps(model, pos[:L], HM, WM)))
            tp.append(timed(lambda: lighting.light_probes(model, pos[:L], HM, WM)))
        say("  %2d lights  shadow_maps %.4f / %.4f / %.4f   light_probes %.4f / %.4f / %.4f   (%.3g rays/s; %.2f of the frame's render)"
            % (L, *stats(ts), *stats(tp), L * HM * WM / stats(ts)[1], stats(ts)[1] / stats(t_view)[1]))
    maps = rl.shadow_maps(model, pos, HM, WM)
    say()

    rays = views.generate_camera_rays(cam, c2w, device=dev)
    packed = rl.pack_lights(lights, dev)
    empty = torch.full_like(maps, float("nan"))
    fixed = R * (3 + 3 + 1 + 3 + 3 + 3) * 4
    say(f"relight of the frame ({R} rows) against {HM} x {WM} maps: ms per call, pairs/s and gathered bytes/s at the median")
    say(f"(rows read once: {fixed / 1e6:.1f} MB; written: 24 + 4 L bytes a row):")
    for L in (1, 4, 16):
        call = lambda m, k: rl.relight(view["fine_rgb"], view["fine_dep"], view["fine_nor"], view["albedo"], rays, packed[:L], m[:L], pcf=k)
        looked = int((call(empty, 1)["visibility"] == 1).sum())
        for k in (1, 3, 5):
            ms = [windowed(lambda: call(maps, k), a.window) for _ in range(a.repeats)]
            med = stats(ms)[1] * 1e-3
            gathered = looked * k * k * 16
            say("  L = %2d  pcf %d   %.3f / %.3f / %.3f ms   %.3g pairs/s   lookups %d of %d pairs (%.0f %%)   gathered %.3g B/s = %.3f of the copy rate"
                % (L, k, *stats(ms), R * L / med, looked, R * L, 100.0 * looked / (R * L), gathered / med,
                   gathered / med / 1e12 / stats(hbm)[1]))
    vis = call(maps, 3)["visibility"]
    say("  visibility of the 16 lights at pcf 3: %.1f %% of the pairs 0, %.1f %% 1, the rest between"
        % (100.0 * float((vis == 0).float().mean()), 100.0 * float((vis == 1).float().mean())))
    say()
    if a.resources and os.path.exists(a.resources):
        text = open(a.resources).read()
        got = {k: re.search(k + r"[^:\n]*:\s*(\d+)", text) for k in ("VGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size", "VGPRs Spill")}
        say("Resources of k_relight (compiler's report, gfx950, -Rpass-analysis=kernel-resource-usage): "
            + ", ".join(f"{k} {m.group(1)}" for k, m in got.items() if m) + ".")
    else:
        say("Resources of k_relight: no compiler report was given (--resources).")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
