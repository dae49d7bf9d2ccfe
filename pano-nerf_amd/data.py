"""Scene folders: metadata, split, pose conversion and on-device ingest of the EXR materials.

``PanoScene`` is the counterpart of ``PanoDataset`` (datasets/pano_datasets.py:7-150) for both splits at once.  The host
reads ``<data_dir>/<meta_file>.json``, converts the Blender poses (``:86-98`` with ``bld_to_wd``, ``:287-295``) and
decodes one EXR file at a time into its stored channel planes (``io_exr.read_exr_planes``); everything per pixel -
channel select, HALF -> fp32, the ``cv2.resize(INTER_AREA)`` block mean at the integer ``factor`` and the per-material
fix-ups (``:100-116``) - is one HIP launch per file (``pn_ingest_image``), so the host never holds more than one file's
raw planes.  The training split becomes a ``DeviceRayPool`` whose colours are the ingested pixels; held-out views come
out in the layouts ``render_image`` and ``evaluate_panorama`` take.

Unpinned: the reference shrinks with cv2 and decodes with the OpenEXR library; neither exists where this package is
built and tested, so the golden (tests/golden/make_dataset_golden.py) stands an fp64 block mean in for ``cv2.resize`` and
this package's reader in for ``read_exr``.  cv2's exact INTER_AREA rounding and codec parity are not checked.

The helpers ``read_meta``, ``split_views``, ``convert_pose`` and ``check_downscale`` need no device.
"""
import json
import math
import os

import numpy as np
import torch

from . import _lib, io_exr
from .rays import DeviceRayPool, Rays, generate_pano_rays, generate_lit_rays

MATERIALS = ("image", "albedo", "normal", "depth")
_KIND = {"image": 0, "albedo": 1, "normal": 2, "depth": 3}  # PN_INGEST_*


def read_meta(data_dir, meta_file="transforms_all"):
    """-> {material: [{file_path, transform_matrix}, ...] or None}; `image` is required, the other lists may be absent."""
    with open(os.path.join(data_dir, meta_file + ".json")) as fp:
        meta = json.load(fp)
    if not meta.get("image"):
        raise ValueError(f"{meta_file}.json has no 'image' list")
    out = {m: (list(meta[m]) if meta.get(m) else None) for m in MATERIALS}
    n = len(out["image"])
    for m in MATERIALS[1:]:
        if out[m] is not None and len(out[m]) != n:
            raise ValueError(f"{meta_file}.json lists {len(out[m])} '{m}' entries for {n} images")
    return out


def split_views(n_views, train_views=None):
    """-> (train list, held-out list) (datasets/pano_datasets.py:55-61): None trains on every view and holds nothing out;
    a list trains on those indices in the given order and holds out all others in ascending order."""
    if train_views is None:
        return list(range(n_views)), []
    train = [int(i) for i in train_views]
    bad = [i for i in train if not 0 <= i < n_views]
    if bad:
        raise ValueError(f"train_views {bad} outside the {n_views} views of the scene")
    return train, [i for i in range(n_views) if i not in train]


def name_switches(data_dir):
    """The reference keys two conversions on the folder path (datasets/pano_datasets.py:89, 112):
    -> (keep_rotation: 'rot' or 'std' in it, pano_normals: 'pano' in it)."""
    return ("rot" in data_dir) or ("std" in data_dir), "pano" in data_dir


def _rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def convert_pose(transform_matrix, keep_rotation):
    """Blender camera matrix -> float32 [4, 4] world pose: rotation R_x(pi/2)^T rm R_x(-pi/2)^T R_x(pi/2) (or the
    identity when the scene's rotations are not kept), translation t R_x(pi/2); fp64 products cast to fp32."""
    mx = np.array(transform_matrix, dtype=np.float32)
    if mx.shape != (4, 4):
        raise ValueError("transform_matrix must be 4x4")
    b2w, w2b = _rot_x(math.pi / 2), _rot_x(-math.pi / 2)
    translate = mx[:3, -1].copy()
    mx[:3, :3] = (b2w.T @ mx[:3, :3] @ w2b.T @ b2w) if keep_rotation else np.eye(3)
    mx[:3, -1] = translate @ b2w
    return mx


def check_downscale(height, width, factor):
    """-> (height // factor, width // factor); a factor that does not divide both sides is not built here."""
    factor = int(factor)
    if factor <= 0:
        raise ValueError(f"{factor} is not positive, please use a positive factor")
    if height % factor or width % factor:
        raise ValueError(f"factor {factor} does not divide the {height} x {width} source: only integer block means "
                         "(cv2.INTER_AREA at a dividing factor) are built here")
    return height // factor, width // factor


def ingest_image(planes, names, material, factor=1, pano_normals=False, normalize_depth=False, near=0.0, far=10.0,
                 device="cuda"):
    """One decoded file -> the [H / f, W / f, C] fp32 device image of `material` (pn_ingest_image, one launch on the
    current stream).  planes: [Hs, n_ch, Ws] float16 / float32 array (numpy, or a device tensor), names: its channels."""
    if material not in _KIND:
        raise ValueError(f"material must be one of {MATERIALS}")
    device = torch.device(device)
    src = torch.as_tensor(planes)
    if src.dtype not in (torch.float16, torch.float32) or src.dim() != 3:
        raise ValueError("planes must be a [Hs, n_ch, Ws] float16 or float32 array")
    hs, n_ch, ws = src.shape
    h, w = check_downscale(hs, ws, factor)
    want = "R" if material == "depth" else "RGB"
    missing = [c for c in want if c not in names]
    if missing:
        raise ValueError(f"the {material} file has no channel {missing} (found {list(names)})")
    ch = [names.index(c) for c in want] + [0] * (3 - len(want))
    src = src.to(device).contiguous()
    out = torch.empty(h, w, 1 if material == "depth" else 3, dtype=torch.float32, device=device)
    flag = pano_normals if material == "normal" else (normalize_depth if material == "depth" else False)
    with torch.cuda.device(device):
        _lib.call("pn_ingest_image", hs, ws, n_ch, int(src.dtype == torch.float16), src.data_ptr(), *ch, int(factor),
                  _KIND[material], int(bool(flag)), float(near), float(far), out.data_ptr(),
                  torch.cuda.current_stream(device).cuda_stream)
    return out


class PanoScene:
    """A scene folder on the device.

    .train          DeviceRayPool over the training views (`.train.sample(B)` is the training batch; `.train.rgbs` the
                    ingested colours); .train_depths / .train_normals / .train_albedos: the other pools or None
    .held_out[i]    (rays [1, H, W, .], hdr [1, H, W, 3], depth [1, H, W, 1], normal, albedo) of held-out view i, a
                    missing material as None
    .env_rays(num)  the light rays of the pool's pixel radius
    """

    def __init__(self, data_dir, factor=4, train_views=None, near=0., far=10., normalize_depth=False,
                 meta_file="transforms_all", device="cuda", white_bkgd=False, keep_rotation=None, pano_normals=None):
        if white_bkgd:
            raise NotImplementedError("white_bkgd composites over the alpha of 4-channel files; no panorama scene has them")
        self.data_dir, self.factor = data_dir, int(factor)
        self.near, self.far, self.normalize_depth = float(near), float(far), bool(normalize_depth)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        by_name = name_switches(data_dir)
        self.keep_rotation = by_name[0] if keep_rotation is None else bool(keep_rotation)
        self.pano_normals = by_name[1] if pano_normals is None else bool(pano_normals)
        self.meta = read_meta(data_dir, meta_file)
        self.train_list, self.held_out_list = split_views(len(self.meta["image"]), train_views)
        self.c2ws = {i: convert_pose(self.meta["image"][i]["transform_matrix"], self.keep_rotation)
                     for i in self.train_list + self.held_out_list}
        train = {m: self._load(m, self.train_list) for m in MATERIALS}
        self.h, self.w = train["image"][0].shape[:2]
        self.train = DeviceRayPool(self.h, self.w, [self.c2ws[i] for i in self.train_list], near=self.near, far=self.far,
                                   device=self.device)
        flat = lambda ims: None if ims is None else torch.cat([x.reshape(-1, x.shape[-1]) for x in ims], 0)
        self.train.rgbs = flat(train["image"])
        self.train_albedos, self.train_normals, self.train_depths = (flat(train[m]) for m in MATERIALS[1:])
        self.radius = self.train.radius
        held = {m: self._load(m, self.held_out_list) for m in MATERIALS}
        self.held_out = []
        for n, i in enumerate(self.held_out_list):
            rays = generate_pano_rays(self.h, self.w, self.c2ws[i], self.near, self.far, device=self.device)
            rays = Rays(*[x.view(1, self.h, self.w, -1) for x in rays])
            mats = [None if held[m] is None else held[m][n].unsqueeze(0) for m in ("image", "depth", "normal", "albedo")]
            self.held_out.append((rays, *mats))

    def _load(self, material, views):
        entries = self.meta[material]
        if entries is None:
            return None
        out = []
        for i in views:
            planes, names, _ = io_exr.read_exr_planes(os.path.join(self.data_dir, entries[i]["file_path"] + ".exr"))
            out.append(ingest_image(planes, names, material, self.factor, self.pano_normals, self.normalize_depth,
                                    self.near, self.far, self.device))
        return out

    def has(self, material):
        return self.meta[material] is not None

    def env_rays(self, num=10, near=0.0, far=10.0):
        return generate_lit_rays(num, self.radius, near, far, device=self.device)
