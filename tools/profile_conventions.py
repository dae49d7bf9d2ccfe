"""GPU cost of the kernels that instantiate the shared projection, tap and SH-basis templates of pn_rays.h / pn_probes.h and
whose own tools need a rendered model for their inputs (tools/profile_views.py, profile_warp.py, profile_volume.py,
profile_sparse_volume.py): the kernels alone, at those tools' shapes, on seeded random inputs.  One process, one JSON line:
name -> [min, median, max] ms of --repeats windows of back-to-back calls between two device events after a warm-up call
(tools/profile_textures.py's windowed).  k_ibl_shade and k_sh_volume_irradiance are timed by tools/profile_ibl.py and
tools/profile_lighting.py --what kernels, which need no model.

    python tools/profile_conventions.py [--repeats 5]
    PN_LIB=<another build of the library> python tools/profile_conventions.py      # as tools/bench_with_lib.py

reproject: a 512 x 1024 panorama into a 480 x 640 pinhole, a 256 cube and a 480 x 480 fisheye frame and back, 2 x 2 subsamples.
warp: one 480 x 640 RGB-D pinhole frame into one other pose of every camera kind.
march: render_volume of a 480 x 640 frame through a 128^3 volume, sh_degree 0 / 1 / 2, dense and sparse (fp32, fp16).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pano_nerf_amd import _lib  # noqa: E402

if os.environ.get("PN_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["PN_LIB"])
from pano_nerf_amd import views, volume  # noqa: E402
from tools.profile_textures import windowed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g)  # noqa: E731
    out = {}

    def t(name, fn, window):
        ms = [windowed(fn, window) for _ in range(a.repeats)]
        out[name] = [round(min(ms), 5), round(float(np.median(ms)), 5), round(max(ms), 5)]

    pano, pin = views.pano_camera(512, 1024), views.perspective_camera(480, 640, fov_x_deg=60.0)
    cube, fish = views.cubemap_camera(256), views.fisheye_camera(480, 480)
    img = rnd(1, 3, 512, 1024)
    for name, dst in (("pinhole", pin), ("cube", cube), ("fisheye", fish)):
        t(f"reproject_pano_to_{name}_s2", lambda: views.reproject(img, pano, dst, None, 2), 20)
        src = views.reproject(img, pano, dst, None, 1)[0]
        t(f"reproject_{name}_to_pano_s2", lambda: views.reproject(src, dst, pano, None, 2), 20)

    depth, rgb = rnd(1, 480, 640) * 2.0 + 0.5, rnd(1, 3, 480, 640)
    p = np.stack([views.look_at([0.3, 0.0, 0.0], [-0.15, 0.0, 0.0]), views.look_at([-0.3, 0.0, 0.0], [0.15, 0.0, 0.0])])
    for name, dst in (("pinhole", pin), ("pano", views.pano_camera(256, 512)), ("cube", views.cubemap_camera(128)), ("fisheye", fish)):
        t(f"warp_pinhole_to_{name}", lambda: views.warp_view(rgb, depth, pin, p[:1], dst, p[1:]), 20)

    pose = views.look_at([0.2, 0.1, 2.5], [0.0, 0.0, 0.0])
    for deg in (0, 1, 2):
        C = 1 + 3 * (deg + 1) ** 2
        data = torch.randn(128, 128, 128, C, device=dev, generator=g)
        data[..., 1:4] += 1.5
        data[..., 0] = (torch.randn(128, 128, 128, device=dev, generator=g) * 12.0 - 6.0).clamp_min(0.0)
        dense = volume.RadianceVolume(data, ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), deg)
        for tag, vol in (("dense", dense), ("sparse_f32", dense.to_sparse(torch.float32)), ("sparse_f16", dense.to_sparse(torch.float16))):
            t(f"march_deg{deg}_{tag}", lambda: volume.render_volume(vol, pin, pose, far=5.0), 5)
        del data, dense
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
