"""Golden vectors for the scene loader (pano_nerf_amd.data) by RUNNING the reference's own PanoDataset
(datasets/pano_datasets.py:7-150) on a small seeded scene folder.

A 5-view scene (16 x 32 source, factor 2; view 0's image holds one NaN and one value of 5000) is written twice, into
folders named `scene_std_pano` (rotations converted, normals flipped) and `plain` (identity rotations, no flip), with
this package's EXR writer; PanoDataset then runs for split='train' and split='val' with num=[0, 2, 3].

Two of the reference's dependencies do not exist where this runs and are stubbed:
  * utils.io_exr.read_exr (the OpenEXR binding)  -> this package's io_exr.read_exr;
  * cv2.resize(..., INTER_AREA)                  -> an fp64 mean over factor x factor blocks, cast to fp32.
So the golden pins the split, the pose conversion, the folder-name switches and the per-material fix-ups, and NOT cv2's
own INTER_AREA rounding or the OpenEXR library's codec: neither can be pinned on a machine without cv2 and OpenEXR.

Build container only (needs a checkout of the reference at REF); stores seeded inputs and the reference's outputs, no
reference code.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dataset_golden.py
"""
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)

import numpy as np  # noqa: E402


def _resize(image, dsize, interpolation=None):
    w, h = dsize
    f = image.shape[0] // h
    assert image.shape[0] == h * f and image.shape[1] == w * f
    img = image.astype(np.float64).reshape(h, f, w, f, -1).mean(axis=(1, 3)).astype(np.float32)
    return img


_cv2 = types.ModuleType("cv2")
_cv2.INTER_AREA = 3
_cv2.resize = _resize
sys.modules["cv2"] = _cv2
sys.modules["Imath"] = types.ModuleType("Imath")
_exr = types.ModuleType("OpenEXR")
_exr.InputFile = _exr.OutputFile = _exr.Header = object
sys.modules["OpenEXR"] = _exr

from scipy.spatial.transform import Rotation  # noqa: E402

from pano_nerf_amd import io_exr  # noqa: E402
import datasets.pano_datasets as pd  # noqa: E402

pd.read_exr = lambda fp: io_exr.read_exr(fp.name)

N, HS, WS, F = 5, 16, 32, 2
TRAIN = [0, 2, 3]
rng = np.random.Generator(np.random.PCG64(53))
src = {"image": (rng.gamma(1.5, 1.0, (N, HS, WS, 3))).astype(np.float32),
       "albedo": rng.uniform(0, 1, (N, HS, WS, 3)).astype(np.float32),
       "normal": rng.uniform(0, 1, (N, HS, WS, 3)).astype(np.float32),
       "depth": rng.uniform(0.5, 12.0, (N, HS, WS, 1)).astype(np.float32)}
src["image"][0, 3, 5, 1] = np.nan
src["image"][0, 8:10, 20:22, 2] = 5000.0
src["image"][1, 0, 0, 0] = -0.5 * 4 - 10.0  # a block whose mean is negative: clips to 0
mats = []
for i in range(N):
    m = np.eye(4)
    m[:3, :3] = Rotation.from_euler("xyz", rng.uniform(-180, 180, 3), degrees=True).as_matrix()
    m[:3, 3] = rng.uniform(-2, 2, 3)
    mats.append(m)
mats = np.array(mats)

out = {"factor": F, "train_views": np.array(TRAIN), "transform_matrices": mats}
out.update({"src_" + k: v for k, v in src.items()})

with tempfile.TemporaryDirectory() as tmp:
    for folder in ("scene_std_pano", "plain"):
        d = os.path.join(tmp, folder)
        os.makedirs(d)
        meta = {}
        for mat, arr in src.items():
            meta[mat] = []
            for i in range(N):
                name = f"{mat}_{i:03d}"
                io_exr.write_exr(os.path.join(d, name + ".exr"), arr[i])
                meta[mat].append({"file_path": name, "transform_matrix": mats[i].tolist()})
        with open(os.path.join(d, "transforms_all.json"), "w") as fp:
            json.dump(meta, fp)
        for split in ("train", "val"):
            for norm in (False, True):
                ds = object.__new__(pd.PanoDataset)
                pd.BaseDataset.__init__(ds, d, split, False, "single_image", F)
                ds.num, ds.num_start, ds.near, ds.far, ds.normalize_depth = TRAIN, 0, 0, 10, norm
                ds.reform_cam, ds.origin, ds.scale, ds.rot = False, None, None, None
                ds._load_renderings()
                ds._generate_rays()
                key = f"{folder}_{split}_"
                if norm:
                    out[key + "depths_normalized"] = np.array(ds.depths)
                    continue
                out[key + "data_list"] = np.array(ds.data_list)
                out[key + "camtoworlds"] = np.array(ds.camtoworlds)
                out[key + "images"] = np.array(ds.images)
                out[key + "albedos"] = np.array(ds.albedos)
                out[key + "normals"] = np.array(ds.normals)
                out[key + "depths"] = np.array(ds.depths)
                out[key + "radii"] = np.array(ds.radii)

assert list(out["plain_val_data_list"]) == [1, 4]
assert all(np.array_equal(c[:3, :3], np.eye(3)) for c in out["plain_train_camtoworlds"])  # (the temporary path is clean)
assert not any(np.array_equal(c[:3, :3], np.eye(3)) for c in out["scene_std_pano_train_camtoworlds"])
assert out["scene_std_pano_train_images"][0].min() == 0 and out["scene_std_pano_train_images"][0].max() == 1000
np.savez_compressed(os.path.join(HERE, "dataset_ref.npz"), **out)
for k, v in out.items():
    print(k, getattr(v, "shape", v), getattr(v, "dtype", ""))
