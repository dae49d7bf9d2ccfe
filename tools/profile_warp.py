"""GPU cost of depth-aware view warping (views.warp_view: pn_warp_splat + pn_warp_resolve) next to what it replaces and
what it resembles.

--what warp: a 512 x 1024 x 3 panorama with its depth (a box room seen from inside, depths 2 - 3.5) warped
    into one 480 x 640 pinhole frame, into one 512 x 1024 panorama, and into 32 pinhole frames in one call, at max_splat 1
    and 4; views.reproject of the same image into the same destination (the same bytes, a gather, no atomics) in the same
    run; the two kernels apart (splat alone on a prepared z-buffer, the z-buffer fill, resolve alone).  Device time from
    events around back-to-back calls after a warm-up, --repeats rounds alternating the legs: median and spread (max - min).
    Atomics are counted, not measured: the k x k pixels of every point that projects, from the same geometry in torch
    (rows a panorama clips at its poles and columns a frame clips are counted as issued: an upper bound within a percent).
--what path: render_path_warped at key_every = 8 against render_path over the same 64 poses at --size (wall time,
    synchronised, alternating), on the seeded model of tools/profile_views.py.

    With --finish also render_path_warped(blend=True, inpaint=True), and the mean absolute difference of consecutive
    "ldr" frames across a rendered pose against that between two warped poses, with and without blend.
--what fill: finishing a warped frame (views.fill_holes: pn_fill_holes; views.blend_warps: pn_warp_blend).  The room gets a
    smooth texture of the world point, so the view from another pose is known analytically.  The panorama is warped into
    a 480 x 640 pinhole frame and a 512 x 1024 panorama at max_splat 4; the holes of that frame, and of the same frame
    with half of its pixels knocked out at random, are filled with and without the depth; two layers of the frame are
    blended.  Device time next to warp_view of the same frame in the same run (alternating, median and spread), the
    launches counted, pn_fill_holes alone on those frames and on frames that are small levels themselves (with --other-lib
    next to a second build, e.g. one with PN_EXTRA=-DPN_FILL_SMALL_TEXELS=0 that gives every level its own launches), bytes computed from the shapes over that time
    against a device-to-device copy measured in the same run, and the mean absolute error against the analytic view over
    the hole pixels and over the frame: the constant `fill`, depth-blind filling (depth=None) and depth-aware filling.

    python tools/profile_warp.py --what warp
    python tools/profile_warp.py --what path --size 480x640 [--finish]
    python tools/profile_warp.py --what fill
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pano_nerf_amd as pn  # noqa: E402
from oracle import pano_oracle as orc  # noqa: E402
from pano_nerf_amd import views, _lib  # noqa: E402
from pano_nerf_amd.cameras import _kind_params  # noqa: E402

HBM_COPY_TB_S = 6.29  # measured float4 copy rate of one MI355X (tools/profile_views.py)


def event_ms(fn, iters):
    """device time per call from HIP events around `iters` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 5), spread=round(xs[-1] - xs[0], 5), all=[round(x, 5) for x in xs])


def room(dev, H=512, W=1024):
    """(image [1, 3, H, W], depth [1, 1, H, W], unit directions [H W, 3]) of a box room of half-size 2 seen from its centre"""
    rays = views.generate_camera_rays(views.pano_camera(H, W), np.eye(4), device=dev)
    d = rays.directions
    depth = (2.0 / d.abs().amax(-1)).view(1, 1, H, W).contiguous()
    g = torch.Generator(device="cpu").manual_seed(0)
    image = torch.rand(1, 3, H, W, generator=g).to(dev)
    return image, depth, d


def count_atomics(d, depth, src, dst, dst_c2ws, max_splat):
    """the k x k pixels of every point that projects (fp32 torch restatement of the header's size; clipping ignored)"""
    dev = d.device
    X = d * depth.reshape(-1, 1)
    a_s = 2 * math.sin(0.5 * math.pi / src.h)
    total = 0
    for m in np.asarray(dst_c2ws, np.float64).reshape(-1, 4, 4):
        R = torch.tensor(m[:3, :3], dtype=torch.float32, device=dev)
        e = (X - torch.tensor(m[:3, 3], dtype=torch.float32, device=dev)) @ R
        rho = e.norm(dim=-1)
        if isinstance(dst, views.PinholeCamera):
            c2p = torch.tensor(np.linalg.inv(np.asarray(dst.pix2cam, np.float64)), dtype=torch.float32, device=dev)
            q = e @ c2p.T
            px, py = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
            ok = (q[:, 2] > 0) & (px >= 0) & (px <= dst.w) & (py >= 0) & (py <= dst.h)
            p2c = torch.tensor(np.asarray(dst.pix2cam, np.float32), device=dev)
            ly, lx = py.floor().clamp(0, dst.h - 2), px.floor().clamp(0, dst.w - 1)

            def unit(yy):
                v = torch.stack([lx + 0.5, yy + 0.5, torch.ones_like(lx)], -1) @ p2c.T
                return v / v.norm(dim=-1, keepdim=True)
            a_d = (unit(ly) - unit(ly + 1)).norm(dim=-1)
        else:
            ok = torch.ones_like(rho, dtype=torch.bool)
            a_d = 2 * math.sin(0.5 * math.pi / dst.h)
        size = depth.reshape(-1) * a_s / (rho * a_d)
        k = size.ceil().clamp(1, max_splat)
        total += int((k * k)[ok].sum().item())
    return total


def warp(repeats, iters):
    dev = torch.device("cuda:0")
    src = views.pano_camera(512, 1024)
    image, depth, dirs = room(dev)
    pin, pano = views.perspective_camera(480, 640, fov_x_deg=60.0), views.pano_camera(512, 1024)
    one = views.look_at([0.3, 0.1, -0.2], [0.0, 0.2, -2.0])
    many = np.stack([views.look_at([0.4 * math.cos(a), 0.1, 0.4 * math.sin(a)], [2 * math.cos(a + 1), 0, 2 * math.sin(a + 1)])
                     for a in np.linspace(0, 2 * np.pi, 32, endpoint=False)])
    pose_pano = np.eye(4)
    pose_pano[:3, 3] = (0.3, 0.1, -0.2)
    rot = one[:3, :3]  # the source pose is the identity
    out = dict(what="warp", repeats=repeats, iters=iters, hbm_copy_tb_per_s=HBM_COPY_TB_S)
    legs = {}
    for name, dst, poses in (("pano_to_pinhole480x640", pin, one), ("pano_to_pano512x1024", pano, pose_pano),
                             ("pano_to_32_pinhole480x640", pin, many)):
        for k in (1, 4):
            legs[f"warp_view_{name}_k{k}"] = (dst, poses, k, (lambda dst=dst, poses=poses, k=k: views.warp_view(
                image, depth, src, np.eye(4), dst, poses, max_splat=k)))
    refs = {"reproject_pano_to_pinhole480x640": lambda: views.reproject(image, src, pin, rotation=rot),
            "reproject_pano_to_pano512x1024": lambda: views.reproject(image, src, pano)}
    # the kernels apart, on the single pinhole frame and on the panorama, max_splat 4
    parts = {}
    (sk, sp), st = _kind_params(src), _lib.stream(dev)
    z = depth.reshape(1, 512, 1024)
    ms = torch.eye(4, device=dev).reshape(1, 16).contiguous()
    keep = []
    for name, dst, poses in (("pinhole480x640", pin, one), ("pano512x1024", pano, pose_pano), ("32_pinhole480x640", pin, many)):
        dk, dp = _kind_params(dst)
        p = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        D = p.shape[0]
        md = torch.from_numpy(p.astype(np.float32).reshape(D, 16)).to(dev)
        zbuf = torch.full((D, dst.h, dst.w), -1, dtype=torch.int64, device=dev)
        o = torch.empty(D, 3, dst.h, dst.w, device=dev)
        dep, cov = torch.empty(D, dst.h, dst.w, device=dev), torch.empty(D, dst.h, dst.w, device=dev)
        idx = torch.empty(D, dst.h, dst.w, dtype=torch.int64, device=dev)
        sn, sc, _, sw = image.stride()
        keep.append((dp, md, zbuf, o, dep, cov, idx))
        parts[f"zbuf_fill_{name}"] = (lambda zbuf=zbuf: zbuf.fill_(-1))  # first: the splats and the resolve see a full one
        for k in (1, 4):
            # the z-buffer is NOT reset between calls: after the first every minimum loses, the atomics are still issued
            parts[f"splat_{name}_k{k}"] = (lambda D=D, dk=dk, dp=dp, md=md, zbuf=zbuf, dst=dst, k=k: _lib.call(
                "pn_warp_splat", 1, sk, 512, 1024, sp.ctypes.data, z.data_ptr(), ms.data_ptr(), D, dk, dst.h, dst.w,
                dp.ctypes.data, md.data_ptr(), k, 1.0, zbuf.data_ptr(), st))
        parts[f"resolve_{name}"] = (lambda D=D, dk=dk, dp=dp, zbuf=zbuf, dst=dst, o=o, dep=dep, idx=idx, cov=cov: _lib.call(
            "pn_warp_resolve", 1, 3, 512, 1024, D, dk, dst.h, dst.w, dp.ctypes.data, zbuf.data_ptr(), image.data_ptr(), sn, sc,
            sw, 0.0, o.data_ptr(), dep.data_ptr(), idx.data_ptr(), cov.data_ptr(), st))
    fns = {**{k: v[3] for k, v in legs.items()}, **refs, **parts}
    for fn in fns.values():  # warm-up of every shape
        fn()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(event_ms(fn, iters))
    out["ms"] = {k: stats(v) for k, v in times.items()}
    # counted work
    n_src = 512 * 1024
    work = {}
    for name, (dst, poses, k, fn) in legs.items():
        D = np.asarray(poses).reshape(-1, 4, 4).shape[0]
        n_dst = D * dst.h * dst.w
        res = fn()
        atomics = count_atomics(dirs, depth, src, dst, poses, k)
        covered = int((res["index"] >= 0).sum().item())
        # depth read; z-buffer filled, hit by the atomics (8 B each), read back; colours gathered; four outputs written
        by = 4 * n_src + 8 * n_dst + 8 * atomics + 8 * n_dst + 12 * covered + (12 + 4 + 8 + 4) * n_dst
        t = out["ms"][name]["median"] * 1e-3
        part = name.replace("warp_view_pano_to_", "splat_")
        ts = out["ms"][part]["median"] * 1e-3
        work[name] = dict(destinations=D, atomics=atomics, covered_share=round(covered / n_dst, 4), bytes=by,
                          tb_per_s=round(by / t / 1e12, 4), atomics_per_s_of_splat=round(atomics / ts, 1),
                          source_points_per_s_of_splat=round(n_src * D / ts, 1))
    for name, dst in (("reproject_pano_to_pinhole480x640", pin), ("reproject_pano_to_pano512x1024", pano)):
        by = 12 * n_src + 16 * dst.h * dst.w
        work[name] = dict(bytes=by, tb_per_s=round(by / (out["ms"][name]["median"] * 1e-3) / 1e12, 4))
    out["work"] = work
    print(json.dumps(out))


def texture(X):
    """a smooth colour [.., 3] of a world point [.., 3]"""
    k = torch.tensor([[1.3, 0.4, -0.7], [-0.5, 1.1, 0.9], [0.8, -1.2, 0.6]], device=X.device)
    return 0.5 + 0.5 * torch.sin(X @ k.T + torch.tensor([0.3, 1.1, 2.0], device=X.device))


def analytic_view(camera, c2w, dev):
    """[1, 3, H, W]: the textured room (half-size 2) seen by a posed camera inside it"""
    rays = views.generate_camera_rays(camera, c2w, device=dev)
    o, d = rays.origins, rays.directions
    t = ((torch.sign(d) * 2.0 - o) / d).amin(-1, keepdim=True)  # the nearest wall along each ray (inf where d = 0)
    return texture(o + t * d).view(1, camera.h, camera.w, 3).permute(0, 3, 1, 2).contiguous()


def fill_levels(H, W):
    sizes = [(H, W)]
    while sizes[-1] != (1, 1):
        sizes.append(((sizes[-1][0] + 1) >> 1, (sizes[-1][1] + 1) >> 1))
    return sizes


def fill_launches(sizes, C):
    """launches of pn_fill_holes: the levels of <= 1024 texels whose planes fit 48 KB of LDS share one (pn_inpaint.hip)"""
    m, floats = len(sizes), 0
    while m > 1 and sizes[m - 1][0] * sizes[m - 1][1] <= 1024 and (floats + (C + 1) * sizes[m - 1][0] * sizes[m - 1][1]) * 4 <= 48 << 10:
        floats += (C + 1) * sizes[m - 1][0] * sizes[m - 1][1]
        m -= 1
    return 2 * (m - 1) + (1 if m < len(sizes) else 0)


def fill_bytes(sizes, C, holes):
    """bytes pn_fill_holes moves for one image, from the shapes (every texel of a level read once per launch that reads
    it; taps into the smaller level counted as that level once), and those of fill_holes' copies of image and depth"""
    n = [h * w for h, w in sizes]
    pull = (4 + 4 + 4 * C) * n[0] + sum(4 * (C + 1) * (n[l - 1] if l > 1 else 0) + 4 * (C + 1) * n[l] for l in range(1, len(n)))
    push = sum(4 * n[l] + 4 * (C + 1) * n[l + 1] for l in range(1, len(n) - 1))
    push += (4 + 4 + 1) * n[0] + 4 * (C + 1) * n[1] + 4 * (C + 1) * holes
    return pull + push, 2 * 4 * (C + 1) * n[0]


def fill(repeats, iters, other_lib=None):
    dev = torch.device("cuda:0")
    src = views.pano_camera(512, 1024)
    _, depth, dirs = room(dev)
    image = texture(dirs * depth.reshape(-1, 1)).view(1, 512, 1024, 3).permute(0, 3, 1, 2).contiguous()
    pin, pano = views.perspective_camera(480, 640, fov_x_deg=60.0), views.pano_camera(512, 1024)
    one = views.look_at([0.3, 0.1, -0.2], [0.0, 0.2, -2.0])
    pose_pano = np.eye(4)
    pose_pano[:3, 3] = (0.3, 0.1, -0.2)
    out = dict(what="fill", repeats=repeats, iters=iters, max_splat=4)
    big = torch.empty(2, 1 << 26, device=dev)  # 2 x 256 MiB
    fns = {"copy_256MiB": lambda: big[1].copy_(big[0])}
    info, errors, raw = {}, {}, []
    g = torch.Generator(device="cpu").manual_seed(1)
    for name, dst, pose in (("pinhole480x640", pin, one), ("pano512x1024", pano, pose_pano)):
        w = views.warp_view(image, depth, src, np.eye(4), dst, pose, max_splat=4)
        img, dep, cov = w["image"], w["depth"], w["coverage"]
        half = cov * (torch.rand(cov.shape, generator=g) < 0.5).to(dev)
        truth = analytic_view(dst, pose, dev)
        raw.append((name, img, dep, cov))
        sizes = fill_levels(dst.h, dst.w)
        fns[f"warp_view_{name}"] = lambda dst=dst, pose=pose: views.warp_view(image, depth, src, np.eye(4), dst, pose, max_splat=4)
        fns[f"fill_holes_{name}_warp_holes"] = lambda img=img, dep=dep, cov=cov, dst=dst: views.fill_holes(img, dep, cov, dst)
        fns[f"fill_holes_{name}_half_holes"] = lambda img=img, dep=dep, half=half, dst=dst: views.fill_holes(img, dep, half, dst)
        fns[f"fill_holes_{name}_warp_holes_no_depth"] = lambda img=img, cov=cov, dst=dst: views.fill_holes(img, None, cov, dst)
        layers, zs = torch.stack([img, img]), torch.stack([dep, dep * 1.01])
        fns[f"blend_warps_{name}_2_layers"] = lambda layers=layers, zs=zs: views.blend_warps(layers, zs, [0.25, 0.75])
        n = dst.h * dst.w
        launches = fill_launches(sizes, 3)
        info[name] = dict(levels_above_frame=len(sizes) - 1, launches_pn_fill_holes=launches,
                          launches_pn_fill_holes_a_launch_per_level=2 * (len(sizes) - 1),
                          launches_fill_holes=launches + 2, hole_share_warp=round(1 - float(cov.mean()), 4),
                          hole_share_half=round(1 - float(half.mean()), 4))
        for k, c in (("warp_holes", cov), ("half_holes", half)):
            kern, copies = fill_bytes(sizes, 3, int((c == 0).sum()))
            info[name][f"bytes_{k}"] = dict(kernels=kern, copies=copies)
        # 2 layers of colours and depth read, the weights, three outputs written
        info[name]["bytes_blend"] = (2 * 16 + 12 + 4 + 4) * n
        # error against the analytic view
        err = {}
        for k, c in (("warp_holes", cov), ("half_holes", half)):
            hole = (c == 0)[0]
            const = torch.where(c[:, None] > 0, img, torch.zeros_like(img))
            blind = views.fill_holes(img, None, c, dst)["image"]
            aware = views.fill_holes(img, dep, c, dst)["image"]
            err[k] = {m: dict(holes=round(float((x - truth).abs().mean(1)[0][hole].mean()), 6),
                              frame=round(float((x - truth).abs().mean()), 6))
                      for m, x in (("constant_fill_0", const), ("depth_blind", blind), ("depth_aware", aware))}
        errors[name] = err
    # pn_fill_holes itself (in place: `known` keeps every call's work the same), on the warped frames and on frames that ARE
    # small levels - what k_fill_small runs in one launch; next to a build with -DPN_FILL_SMALL_TEXELS=0 (a launch per level)
    libs = {"": _lib.load()}
    if other_lib:
        lib = ctypes.CDLL(os.path.abspath(other_lib))
        for fn_name in ("pn_fill_holes", "pn_fill_holes_work_floats"):
            res, args = _lib.SIGNATURES[fn_name]
            getattr(lib, fn_name).restype = _lib._CODES[res]
            getattr(lib, fn_name).argtypes = [_lib._CODES[c] for c in args]
        libs["_per_level_launches"] = lib
    st = _lib.stream(dev)
    for name, x, z, c in raw + [(f"small{h}x{w_}", torch.rand(1, 3, h, w_, device=dev), 1 + torch.rand(1, h, w_, device=dev),
                                 (torch.rand(1, h, w_, device=dev) < 0.5).float()) for h, w_ in ((15, 20), (16, 32), (30, 40))]:
        h, w_ = x.shape[2:]
        x, z = x.clone(), z.reshape(1, h, w_).clone()
        work = torch.empty(int(libs[""].pn_fill_holes_work_floats(1, 3, h, w_, 32)), device=dev)
        f = torch.empty(1, h, w_, dtype=torch.uint8, device=dev)
        for suffix, lib in libs.items():
            def call(lib=lib, x=x, z=z, c=c, f=f, work=work, h=h, w_=w_):
                _lib.check(lib.pn_fill_holes(1, 3, h, w_, x.data_ptr(), z.data_ptr(), c.data_ptr(), None, 0, 0.05, 32, f.data_ptr(),
                                             work.data_ptr(), work.numel(), st), "pn_fill_holes")
            fns[f"pn_fill_holes_{name}{suffix}"] = call
    for fn in fns.values():
        fn()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(event_ms(fn, iters))
    out["ms"] = {k: stats(v) for k, v in times.items()}
    copy_tb = 2 * big[0].numel() * 4 / (out["ms"]["copy_256MiB"]["median"] * 1e-3) / 1e12
    out["hbm_copy_tb_per_s_this_run"] = round(copy_tb, 3)
    for name in info:
        for k in ("warp_holes", "half_holes"):
            b = info[name][f"bytes_{k}"]
            t = out["ms"][f"fill_holes_{name}_{k}"]["median"] * 1e-3
            b["tb_per_s"] = round((b["kernels"] + b["copies"]) / t / 1e12, 4)
            b["ms_at_copy_rate"] = round((b["kernels"] + b["copies"]) / copy_tb / 1e9, 5)
        t = out["ms"][f"blend_warps_{name}_2_layers"]["median"] * 1e-3
        info[name]["blend_tb_per_s"] = round(info[name]["bytes_blend"] / t / 1e12, 4)
    out["frames"] = info
    out["mean_abs_error_against_the_analytic_view"] = errors
    print(json.dumps(out))


def path(size, repeats, finish=False):
    H, W = (int(v) for v in size.split("x"))
    model = pn.PanoMipNeRF(rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    model.mlp.load_state_dict(orc.init_params(4, 5))
    model = model.cuda()
    cam = views.perspective_camera(H, W, fov_x_deg=60.0)
    poses = np.stack([views.look_at([0.5 * math.sin(a), 0.1 * math.sin(2 * a), 2.5 - 0.3 * (1 - math.cos(a))], [0, 0, 0])
                      for a in np.linspace(0, 1.5, 64)])
    legs = {"render_path": lambda: views.render_path(model, cam, poses, kinds=("ldr", "depth")),
            "render_path_warped_key8": lambda: views.render_path_warped(model, cam, poses, 8, kinds=("ldr", "depth"))}
    if finish:
        legs["render_path_warped_key8_blend_inpaint"] = lambda: views.render_path_warped(
            model, cam, poses, 8, kinds=("ldr", "depth"), blend=True, inpaint=True)
    views.render_view(model, views.perspective_camera(48, 64, fov_x_deg=60.0), poses[0], outputs=("rgb", "depth"))
    views.render_path_warped(model, views.perspective_camera(48, 64, fov_x_deg=60.0), poses[:3], 2)
    times = {k: [] for k in legs}
    cov = None
    for _ in range(repeats):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
            if "coverage" in r:
                cov = float(r["coverage"].mean())
    out = dict(what="path", size=size, poses=64, key_every=8, rendered=9, repeats=repeats,
               seconds={k: stats(v) for k, v in times.items()}, mean_coverage=round(cov, 4))
    out["frames_per_s"] = {k: round(64 / v["median"], 3) for k, v in out["seconds"].items()}
    if finish:  # how much an "ldr" frame jumps when a rendered pose arrives, against a step between two warped poses
        jumps = {}
        for name, kw in (("default", {}), ("blend", dict(blend=True)), ("blend_inpaint", dict(blend=True, inpaint=True))):
            ldr = views.render_path_warped(model, cam, poses, 8, kinds=("ldr",), **kw)["ldr"].float()
            step = (ldr[1:] - ldr[:-1]).abs().mean((1, 2, 3))  # step[i]: frame i -> i + 1, in 8-bit levels
            into_key = [i - 1 for i in range(8, 64, 8)]
            within = [i for i in range(63) if (i + 1) % 8 and i % 8]
            jumps[name] = dict(into_a_rendered_pose=round(float(step[into_key].mean()), 4),
                               between_warped_poses=round(float(step[within].mean()), 4))
        out["mean_abs_ldr_step_in_8bit_levels"] = jumps
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("warp", "path", "fill"), default="warp")
    ap.add_argument("--finish", action="store_true", help="--what path: also blend=True, inpaint=True and the steps across a key")
    ap.add_argument("--size", default="480x640")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--other-lib", help="--what fill: a second build of the library whose pn_fill_holes is timed next to this one")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/profile_warp.py measures on a HIP device; none is available")
    if a.what == "warp":
        warp(a.repeats, a.iters)
    elif a.what == "fill":
        fill(a.repeats, a.iters, a.other_lib)
    else:
        path(a.size, a.repeats, a.finish)
