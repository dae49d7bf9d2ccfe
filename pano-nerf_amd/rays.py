"""Ray containers and on-device ray generation.

``Rays`` is the reference's batch container (datasets/base_datasets.py:13-16).  ``generate_pano_rays``
and ``generate_lit_rays`` stand in for ``PanoDataset._generate_rays`` / ``.generate_lit_rays``
(datasets/pano_datasets.py:152-216, 218-263; == utils/sampling.py:5-38) and run as HIP kernels, so a
ray pool can be regenerated in HBM from (camera, pixel) instead of being shipped from the host.

``CameraRig`` is a camera model (cameras.py) with the poses of n cameras on the device; ``CameraRig.sample`` is the one
place the batch samplers of ``pn_cameras.hip`` are called from.  ``RayPool`` draws training batches from a rig;
``DeviceRayPool`` (panoramas) and ``PerspectiveRayPool`` (pinholes) build the rig from their own arguments.
"""
import collections

import numpy as np
import torch

from . import _lib
from .cameras import PanoCamera, PinholeCamera, _camera, _c2w_stack, _kind_params

Rays = collections.namedtuple(
    "Rays", ("origins", "directions", "viewdirs", "radii", "lossmult", "near", "far", "noise_var"))
Rays_keys = Rays._fields
_DIMS = (3, 3, 3, 1, 1, 1, 1, 1)


def namedtuple_map(fn, tup):
    return type(tup)(*map(fn, tup))


def _cuda_device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("pano_nerf_amd generates rays on a HIP device only (got %s); there is no CPU fallback" % dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def generate_pano_rays(h, w, c2w, near=0.0, far=10.0, device="cuda"):
    """One equirectangular camera -> Rays of [h*w, C] fp32 device tensors (row-major pixels)."""
    device = torch.device(device)
    c = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(-1))
    if c.size != 16:
        raise ValueError("c2w must be a 4x4 matrix")
    out = [torch.empty(h * w, d, dtype=torch.float32, device=device) for d in _DIMS]
    with torch.cuda.device(device):
        _lib.call("pn_raygen_pano", int(h), int(w), c.ctypes.data, float(near), float(far),
                  *[t.data_ptr() for t in out], _lib.stream(device))
    return Rays(*out)


def pano_pixel_radius(rays):
    """The constant pixel radius of a pano (datasets/pano_datasets.py:215)."""
    return float(rays.radii[0, 0])


def generate_lit_rays(num, radius, near=0.0, far=10.0, device="cuda"):
    """`num` golden-spiral light rays as fp16 tensors, like the reference's env_rays."""
    device = torch.device(device)
    buf = torch.empty(14 * num, dtype=torch.float16, device=device)
    with torch.cuda.device(device):
        _lib.call("pn_lit_rays", int(num), float(radius), float(near), float(far), buf.data_ptr(), _lib.stream(device))
    v3 = buf[:9 * num].view(3, num, 3)
    s = buf[9 * num:].view(5, num, 1)
    return Rays(v3[0], v3[1], v3[2], s[0], s[1], s[2], s[3], s[4])


def rearrange_render_image(rays, chunk_size=4096):
    """models/mip.py:530-547: flatten [1,H,W,C] rays and slice into chunks."""
    flat = [getattr(rays, k).reshape(-1, getattr(rays, k).shape[-1]) for k in Rays_keys]
    val_mask = flat[-3]
    n = flat[0].shape[0]
    chunks = [Rays(*[a[i:i + chunk_size] for a in flat]) for i in range(0, n, chunk_size)]
    return chunks, val_mask


class CameraRig:
    """n cameras of one model (a camera of cameras.py) with their poses c2ws [n, 4, 4] on the device: c2ws [n, 16] fp32 and, for a pinhole, the tiled pix2cams [n, 9]; a cube, fisheye or stereo-panorama camera keeps its host
    parameter block.  Row r of the rig is pixel r % (H W), row-major, of camera r // (H W)."""

    def __init__(self, camera, c2ws, device="cuda"):
        self.camera = _camera(camera)
        self.h, self.w = camera.h, camera.w
        self.device = _cuda_device(device)
        self.c2ws = torch.as_tensor(c2ws, dtype=torch.float32).reshape(-1, 16).to(self.device).contiguous()
        n = self.n_cam = self.c2ws.shape[0]
        # the entry point and its arguments before idx and between idx and near (include/panonerf_hip.h)
        if isinstance(camera, PanoCamera):
            self._entry, self._head, self._mats = "pn_sample_pano_rays", (n, self.h, self.w), (self.c2ws.data_ptr(),)
        elif isinstance(camera, PinholeCamera):
            p = np.tile(np.asarray(camera.pix2cam, np.float32).reshape(1, 9), (n, 1))
            self.pix2cams = torch.from_numpy(p).to(self.device)
            self._entry, self._head = "pn_sample_pinhole_rays", (n, self.h, self.w)
            self._mats = (self.pix2cams.data_ptr(), self.c2ws.data_ptr())
        else:
            kind, self._params = _kind_params(camera)
            self._entry, self._head = "pn_sample_camera_rays", (n, kind, self.h, self.w, self._params.ctypes.data)
            self._mats = (self.c2ws.data_ptr(),)

    def __len__(self):
        return self.n_cam * self.h * self.w

    def sample(self, idx, near, far, rgb_pool=None):
        """(Rays, rgb): the rays of the rows idx [B] (int64, contiguous, on the device), regenerated by one kernel, and
        rgb_pool[idx] ([len(rig), 3] fp32 target colours) or None.  A row outside the rig reads row 0."""
        dev = self.device
        B = int(idx.numel())
        with torch.no_grad(), torch.cuda.device(dev):
            outs = [torch.empty(B, d, dtype=torch.float32, device=dev) for d in _DIMS]
            rgb = torch.empty(B, 3, dtype=torch.float32, device=dev) if rgb_pool is not None else None
            _lib.call(self._entry, B, *self._head, idx.data_ptr(), *self._mats, float(near), float(far), _lib.ptr(rgb_pool),
                      *[x.data_ptr() for x in outs], _lib.ptr(rgb), _lib.stream(dev))
        return Rays(*outs), rgb


class RayPool:
    """Batch sampler over the pixels of a rig's cameras.  NO ray pool is stored: a batch is one ``torch.randint`` over
    (camera, pixel) plus one kernel that REGENERATES the rays of the drawn pixels from the camera matrices (56 B/ray of
    HBM and of reads saved; nothing crosses PCIe per step).  Only the target colours ``rgbs`` ([n_cam*H*W, 3], optional:
    ``images`` = [H, W, 3] arrays per camera) are kept and gathered."""

    def __init__(self, rig, images=None, near=0.0, far=10.0):
        self.rig = rig
        self.camera, self.device, self.c2ws = rig.camera, rig.device, rig.c2ws
        self.h, self.w, self.n_cam = rig.h, rig.w, rig.n_cam
        self.near, self.far = float(near), float(far)
        self.rgbs = None
        if images is not None:
            self.rgbs = torch.cat([torch.as_tensor(im, dtype=torch.float32).reshape(-1, 3) for im in images], 0).to(self.device)
            if self.rgbs.shape[0] != len(self):
                raise ValueError("images must be [H, W, 3] per camera")

    def __len__(self):
        return len(self.rig)

    @property
    def rays(self):
        """The materialised pool (camera-major, row-major pixels) - for tests and one-off uses; NOT cached."""
        return self.take(torch.arange(len(self), dtype=torch.int64, device=self.device))[0]

    def take(self, idx):
        """Rays (and target colours) of the pool rows `idx` (int64 device tensor, row = camera * H * W + pixel)."""
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous()
        return self.rig.sample(idx, self.near, self.far, self.rgbs)

    def sample(self, batch_size, generator=None):
        """-> (Rays of [B, C], rgb [B, 3] or None), all on the device."""
        idx = torch.randint(0, len(self), (int(batch_size),), device=self.device, generator=generator)
        return self.take(idx)


class PerspectiveRayPool(RayPool):
    """RayPool over a set of pinhole cameras sharing one PinholeCamera, for Blender- or Multicam-style data: a batch is
    one pn_sample_pinhole_rays."""

    def __init__(self, camera, c2ws, images=None, near=0.0, far=10.0, device="cuda"):
        if not isinstance(camera, PinholeCamera):
            raise ValueError("camera must come from perspective_camera")
        self.c2ws_host = _c2w_stack(c2ws).astype(np.float32)
        super().__init__(CameraRig(camera, self.c2ws_host, device), images, near, far)
        self.pix2cams = self.rig.pix2cams


class DeviceRayPool(RayPool):
    """RayPool over a set of equirectangular cameras: a batch is one ``pn_sample_pano_rays``, which has
    the arithmetic of ``pn_raygen_pano`` - bit-identical to a gather out of the materialised pool.

    Stands in for the reference's flattened numpy ray pool and its 28 DataLoader workers
    (datasets/pano_datasets.py:133-150, 271-275; systems/base_system.py:89-96).  ``images`` are [H, W, 3] HDR arrays.
    """

    def __init__(self, height, width, c2ws, images=None, near=0.0, far=10.0, device="cuda"):
        self.c2ws_host = np.stack([np.asarray(c, dtype=np.float32).reshape(4, 4) for c in c2ws], 0)
        super().__init__(CameraRig(PanoCamera(int(height), int(width)), self.c2ws_host, device), images, near, far)
        # the constant pixel radius of the pano (datasets/pano_datasets.py:215): the light rays carry it
        self.radius = pano_pixel_radius(self.take(torch.zeros(1, dtype=torch.int64, device=self.device))[0])

    @property
    def rays(self):
        """The materialised pool (camera-major, row-major pixels) - for tests and one-off uses; NOT cached."""
        pools = [generate_pano_rays(self.h, self.w, c, self.near, self.far, device=self.device) for c in self.c2ws_host]
        return Rays(*[torch.cat([getattr(p, k) for p in pools], 0) for k in Rays_keys])

    def lit_rays(self, num=10, near=0.0, far=10.0):
        return generate_lit_rays(num, self.radius, near, far, device=self.device)
