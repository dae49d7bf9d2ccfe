"""Cost of the input side (scene folder -> Trainer) next to bench.py, on one MI355X.

    python tools/profile_train.py scene DIR                     # write a 3-view 512 x 1024 scene folder of bench.py's radiance
    python tools/profile_train.py ingest DIR                    # per-view load time of that folder; pn_ingest_image alone
    python tools/profile_train.py fit DIR --batch 4096 --steps 20 --warmup 5

`scene` writes one ZIP / HALF, one ZIP / FLOAT and one uncompressed FLOAT image with bench.py's camera positions, so that
`fit` runs bench.py's workload from files.  `fit` times Trainer.training_step - the loop Trainer.fit runs - over `--steps`
steps after `--warmup` (the graph capture and its check happen in the first of them) with device events around the whole
window and no readback inside it (log_every_n_step 0); one JSON line.  Run it alternating with bench.py at the same size
(profiles/train_fit_rate.txt).  `ingest` prints host decode and upload + kernel seconds per view, and the kernel on a
2048 x 4096 x 3 source at factor 4: 50 back-to-back launches between two events, so the figure includes whatever the
Python call costs beyond the kernel and is a lower bound of the kernel's rate.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pano_nerf_amd as pn  # noqa: E402
from pano_nerf_amd import config, data, io_exr  # noqa: E402

FORMATS = [dict(compression="zip", half=True), dict(compression="zip"), dict()]
B2W = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])  # R_x(pi / 2): the loader multiplies positions by it


def write_scene(folder, h=512, w=1024):
    import bench
    os.makedirs(folder, exist_ok=True)
    g = torch.Generator().manual_seed(4)
    meta = {"image": []}
    for i in range(3):
        t = (torch.rand(3, generator=g) - 0.5).numpy().astype(np.float64)
        m = np.eye(4, dtype=np.float32)
        m[:3, 3] = t
        rays = pn.generate_pano_rays(h, w, m)
        img = bench.analytic_radiance(rays.viewdirs, rays.origins).reshape(h, w, 3).cpu().numpy()
        io_exr.write_exr(os.path.join(folder, f"im{i}.exr"), img, **FORMATS[i])
        mb = np.eye(4)
        mb[:3, 3] = t @ B2W.T
        meta["image"].append({"file_path": f"im{i}", "transform_matrix": mb.tolist()})
    with open(os.path.join(folder, "transforms_all.json"), "w") as fp:
        json.dump(meta, fp)


def ingest(folder):
    for i in range(3):
        name = os.path.join(folder, f"im{i}.exr")
        t0 = time.perf_counter()
        planes, names, types = io_exr.read_exr_planes(name)
        t1 = time.perf_counter()
        data.ingest_image(planes, names, "image", 1)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        print(json.dumps({"what": "load_view", "view": i, "format": FORMATS[i], "pixel_type": types[0],
                          "file_bytes": os.path.getsize(name), "decode_s": t1 - t0, "upload_and_kernel_s": t2 - t1}))
    for dt, name in ((torch.float32, "float"), (torch.float16, "half")):
        src = (torch.rand(2048, 3, 4096, device="cuda") * 4).to(dt)
        for _ in range(3):
            data.ingest_image(src, ["B", "G", "R"], "image", 4)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            data.ingest_image(src, ["B", "G", "R"], "image", 4)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 50 * 1e3
        nbytes = src.numel() * src.element_size() + 512 * 1024 * 3 * 4
        print(json.dumps({"what": "ingest_kernel", "source": f"2048x4096x3 {name}", "factor": 4, "us_per_call": us,
                          "GBps": nbytes / us / 1e3}))


def fit(folder, batch, steps, warmup):
    hp = config.finalize(pn.load_config(None, ["train.factor", "1", "nerf.num_samples", "128", "train.batch_size", str(batch),
                                               "log_every_n_step", "0"]), out_dir=os.path.join(folder, "_out"))
    t0 = time.perf_counter()
    scene = pn.PanoScene(folder, factor=1, train_views=None, keep_rotation=False, pano_normals=False)
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    tr = pn.Trainer(hp, scene)
    for _ in range(warmup):
        tr.training_step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        loss = tr.training_step()
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - w0
    ms = e0.elapsed_time(e1)
    print(json.dumps({"what": "fit", "batch": batch, "steps": steps, "warmup": warmup,
                      "rays_per_s_events": batch * steps / (ms / 1e3), "rays_per_s_wall": batch * steps / wall,
                      "ms_per_step": ms / steps, "loss": float(loss),
                      "launch": "hip-graph replay" if tr._graphs.get(True) else "eager",
                      "replay_check": tr.replay_checks.get(True), "scene_load_s": load_s,
                      "views": len(scene.train_list), "pool": [scene.h, scene.w]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("scene", "ingest", "fit"))
    ap.add_argument("folder")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.what == "scene":
        write_scene(a.folder)
    elif a.what == "ingest":
        ingest(a.folder)
    else:
        fit(a.folder, a.batch, a.steps, a.warmup)
