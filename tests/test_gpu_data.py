"""The device ingest kernel (pn_ingest_image) and the scene loader against the reference's PanoDataset
(tests/golden/make_dataset_golden.py -> dataset_ref.npz; cv2.resize stood in for by an fp64 block mean there).

The tolerance is derived, not measured.  The kernel accumulates the f^2 terms of a block in fp32 and divides once; the
reference is the fp64 mean rounded to fp32:

    |got - ref| <= f^2 2^-24 mean|x| over the block + 2^-24 |ref|

A fix-up's slope carries the bound through (x 2 for `normal`, x 1 / (far - near) for normalised depth) and adds one more
2^-24 |ref| for its own rounding; clipping is 1-Lipschitz.  For HALF files the source is the half-rounded array."""
import json
import os

import numpy as np
import pytest
import torch

import pano_nerf_amd as pn
from pano_nerf_amd import data, io_exr

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_ref.npz"))
U = 2.0 ** -24
F = int(GOLD["factor"])


def planes_of(img, half):
    """[H, W, C] -> ([H, C, W] planes in stored (alphabetical) order, names)."""
    names = ["B", "G", "R"] if img.shape[2] == 3 else ["R"]
    order = [2, 1, 0] if img.shape[2] == 3 else [0]
    p = np.ascontiguousarray(img[:, :, order].transpose(0, 2, 1))
    return (p.astype(np.float16) if half else p), names


def block_stats(x, f):
    """fp64 (mean, mean |.|) over f x f blocks of [H, W, C]."""
    h, w, c = x.shape
    b = x.astype(np.float64).reshape(h // f, f, w // f, f, c)
    return b.mean(axis=(1, 3)), np.abs(b).mean(axis=(1, 3))


def check(got, ref, src, f, slope=1.0, extra=0, what=""):
    mean, mabs = block_stats(src, f)
    mean, mabs = mean[..., :ref.shape[-1]], mabs[..., :ref.shape[-1]]
    ref = ref.astype(np.float64)
    bound = slope * (f * f * U * mabs + U * np.abs(mean)) + extra * U * np.abs(ref)
    nan = np.isnan(mabs)
    bound[nan] = 0.0  # a block with a NaN: the fix-up's value, exactly
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all() or np.array_equal(np.isnan(got), np.isnan(ref)), what
    worst = float(np.nanmax(err / np.maximum(bound, 1e-300) * (err > 0)))
    print(f"{what}: worst |err| / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)


@pytest.mark.parametrize("half", [False, True], ids=["float", "half"])
@pytest.mark.parametrize("folder", ["scene_std_pano", "plain"])
def test_ingest_reproduces_the_reference_loader(folder, half):
    pano = folder == "scene_std_pano"
    lists = {s: GOLD[f"{folder}_{s}_data_list"] for s in ("train", "val")}
    for mat, key in (("image", "images"), ("albedo", "albedos"), ("normal", "normals"), ("depth", "depths"),
                     ("depth", "depths_normalized")):
        for split in ("train", "val"):
            for n, i in enumerate(lists[split]):
                src = GOLD["src_" + mat][i]
                planes, names = planes_of(src, half)
                seen = planes.astype(np.float32).transpose(0, 2, 1)[:, :, ::-1] if src.shape[2] == 3 else \
                    planes.astype(np.float32).transpose(0, 2, 1)
                norm = key == "depths_normalized"
                got = data.ingest_image(planes, names, mat, F, pano_normals=pano, normalize_depth=norm, near=0.0, far=10.0)
                got = got.cpu().numpy()
                ref = GOLD[f"{folder}_{split}_{key}"][n]
                assert got.shape == ref.shape and got.dtype == np.float32
                if half and mat == "image":
                    # the reference ran on the FLOAT files: its image of the half-rounded source is the same fix-up of the
                    # half-rounded block mean
                    m, _ = block_stats(seen, F)
                    ref = np.clip(np.nan_to_num(m.astype(np.float32), nan=0), 0, 1000)
                elif half:
                    m, _ = block_stats(seen, F)
                    m = m.astype(np.float32)
                    if mat == "normal":
                        ref = m.astype(np.float64) * 2 - 1
                        ref = ref * np.array([-1.0, 1.0, -1.0]) if pano else ref
                    elif norm:
                        ref = (np.clip(m[:, :, :1], 0, 10) - 0) / (10 - 0)
                    else:
                        ref = m[:, :, :ref.shape[2]]
                slope, extra = (2.0, 1) if mat == "normal" else ((0.1, 1) if norm else (1.0, 0))
                check(got, ref, seen, F, slope, extra, f"{folder}/{split}/{key}[{n}] {'half' if half else 'float'}")


def test_fixups_nan_and_clip():
    src = GOLD["src_image"][0]
    assert np.isnan(src).sum() == 1 and (src == 5000).sum() == 4
    planes, names = planes_of(src, False)
    got = data.ingest_image(planes, names, "image", F).cpu().numpy()
    ref = GOLD["plain_train_images"][0]
    y, x, c = np.argwhere(np.isnan(src))[0]
    assert got[y // F, x // F, c] == 0.0 == ref[y // F, x // F, c]
    assert got.max() == 1000.0 and np.array_equal(got == 1000.0, ref == 1000.0) and (got == 1000.0).sum() == 1
    assert got.min() >= 0.0
    # depth: NaN stays NaN through the clip, out-of-range values end on the bounds
    d = np.full((2, 1, 2), 3.0, np.float32)
    d[0, 0, 0], d[0, 0, 1], d[1, 0, 0] = np.nan, 50.0, -4.0
    out = data.ingest_image(d, ["R"], "depth", 1, normalize_depth=True, near=1.0, far=5.0).cpu().numpy()[:, :, 0]
    assert np.isnan(out[0, 0]) and out[0, 1] == 1.0 and out[1, 0] == 0.0 and out[1, 1] == 0.5


def test_bad_requests_raise_on_the_host():
    p = np.zeros((6, 3, 8), np.float32)
    with pytest.raises(ValueError):
        data.ingest_image(p, ["B", "G", "R"], "image", 4)  # 4 does not divide 6
    with pytest.raises(ValueError):
        data.ingest_image(p, ["A", "B", "G"], "image", 2)  # no R channel
    with pytest.raises(ValueError):
        data.ingest_image(p.astype(np.float64), ["B", "G", "R"], "image", 2)


@pytest.mark.parametrize("half", [False, True], ids=["float", "half"])
def test_full_size_property(half):
    """1024 x 2048, factor 4: agrees with a torch fp64 avg_pool2d under the same bound; two launches give the same bits."""
    g = torch.Generator().manual_seed(12)
    src = torch.randn(1024, 4, 2048, generator=g) * 3 + 0.5  # 4 planes: A, B, G, R
    if half:
        src = src.half()
    dev = src.cuda()
    a = data.ingest_image(dev, ["A", "B", "G", "R"], "albedo", 4)
    b = data.ingest_image(dev, ["A", "B", "G", "R"], "albedo", 4)
    torch.cuda.synchronize()
    assert a.shape == (256, 512, 3) and torch.equal(a, b)
    x = src.double()[:, [3, 2, 1], :].permute(1, 0, 2).unsqueeze(0)  # [1, RGB, H, W]
    ref = torch.nn.functional.avg_pool2d(x, 4)[0].permute(1, 2, 0).numpy()
    seen = src.float().numpy()[:, [3, 2, 1], :].transpose(0, 2, 1)
    check(a.cpu().numpy(), ref, seen, 4, what=f"1024x2048 f=4 {'half' if half else 'float'}")
    # other factors take the 2-wide and the scalar load paths
    for f in (2, 1, 8):
        small = dev[:64 * f, :, :64 * f].contiguous()
        got = data.ingest_image(small, ["A", "B", "G", "R"], "albedo", f).cpu().numpy()
        sx = src[:64 * f, :, :64 * f].double()[:, [3, 2, 1], :].permute(1, 0, 2).unsqueeze(0)
        check(got, torch.nn.functional.avg_pool2d(sx, f)[0].permute(1, 2, 0).numpy(), seen[:64 * f, :64 * f], f, what=f"f={f}")


def write_scene(folder, half_zip_views=(1, 3)):
    os.makedirs(folder, exist_ok=True)
    meta = {}
    for mat in data.MATERIALS:
        meta[mat] = []
        for i, arr in enumerate(GOLD["src_" + mat]):
            name = f"{mat}_{i:03d}"
            kw = dict(compression="zip") if i in half_zip_views else {}  # FLOAT throughout: the golden ran on FLOAT files
            io_exr.write_exr(os.path.join(folder, name + ".exr"), arr, **kw)
            meta[mat].append({"file_path": name, "transform_matrix": GOLD["transform_matrices"][i].tolist()})
    with open(os.path.join(folder, "transforms_all.json"), "w") as fp:
        json.dump(meta, fp)


@pytest.mark.parametrize("folder", ["scene_std_pano", "plain"])
def test_scene_pools_and_sampling(tmp_path, folder):
    d = str(tmp_path / folder)
    write_scene(d)
    keep, pano = folder == "scene_std_pano", folder == "scene_std_pano"
    train_views = [int(i) for i in GOLD["train_views"]]
    scene = pn.PanoScene(d, factor=F, train_views=train_views, keep_rotation=keep, pano_normals=pano)
    assert scene.train_list == train_views and scene.held_out_list == [1, 4]
    assert (scene.h, scene.w) == (8, 16) and len(scene.train) == 3 * 8 * 16
    cams = GOLD[f"{folder}_train_camtoworlds"]
    assert np.abs(scene.train.c2ws_host - cams).max() <= 1e-6
    assert abs(scene.radius - float(GOLD[f"{folder}_train_radii"])) <= 1e-6 * float(GOLD[f"{folder}_train_radii"])
    for pool, key, slope in ((scene.train.rgbs, "images", 1), (scene.train_albedos, "albedos", 1),
                             (scene.train_normals, "normals", 2), (scene.train_depths, "depths", 1)):
        ref = GOLD[f"{folder}_train_{key}"]
        got = pool.cpu().numpy().reshape(ref.shape)
        assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())  # (the tight bound is checked per file above)
    # a batch = rows of the materialised pool of the converted poses, bit for bit; colours = the ingested pixels
    full = scene.train.rays
    torch.manual_seed(3)
    idx = torch.randint(0, len(scene.train), (200,), device=scene.device)
    torch.manual_seed(3)
    rays, rgb = scene.train.sample(200)
    for k in pn.Rays_keys:
        assert torch.equal(getattr(rays, k), getattr(full, k)[idx]), k
    assert torch.equal(rgb, scene.train.rgbs[idx])
    for n, c2w in enumerate(scene.train.c2ws_host):
        one = pn.generate_pano_rays(8, 16, c2w, 0.0, 10.0)
        assert torch.equal(one.directions, full.directions[n * 128:(n + 1) * 128])
    # held-out views in render_image / evaluate_panorama layouts
    assert len(scene.held_out) == 2
    rays, hdr, depth, normal, albedo = scene.held_out[1]
    assert rays.origins.shape == (1, 8, 16, 3) and hdr.shape == (1, 8, 16, 3) and depth.shape == (1, 8, 16, 1)
    assert normal.shape == albedo.shape == (1, 8, 16, 3)
    assert np.abs(hdr[0].cpu().numpy() - GOLD[f"{folder}_val_images"][1]).max() <= 1e-5 * 1000
    want = pn.generate_pano_rays(8, 16, GOLD[f"{folder}_val_camtoworlds"][1], 0.0, 10.0)
    assert np.abs(rays.directions.reshape(-1, 3).cpu().numpy() - want.directions.cpu().numpy()).max() <= 2e-6
    env = scene.env_rays(10)
    assert env.directions.shape == (10, 3) and env.directions.dtype == torch.float16


def test_missing_materials_and_white_bkgd(tmp_path):
    d = str(tmp_path / "plain")
    write_scene(d)
    meta = json.load(open(os.path.join(d, "transforms_all.json")))
    del meta["albedo"], meta["depth"]
    json.dump(meta, open(os.path.join(d, "transforms_all.json"), "w"))
    scene = pn.PanoScene(d, factor=F, train_views=[0, 1, 2, 3], keep_rotation=False, pano_normals=False)
    assert scene.train_albedos is None and scene.train_depths is None and scene.train_normals is not None
    assert not scene.has("albedo") and scene.has("normal")
    _, hdr, depth, normal, albedo = scene.held_out[0]
    assert depth is None and albedo is None and normal is not None
    everything = pn.PanoScene(d, factor=F, keep_rotation=False, pano_normals=False)
    assert everything.held_out == [] and len(everything.train) == 5 * 128
    with pytest.raises(NotImplementedError):
        pn.PanoScene(d, factor=F, white_bkgd=True)
    with pytest.raises(ValueError):
        pn.PanoScene(d, factor=3)
