"""The field baked into a radiance volume, and that volume ray-marched with no network in the loop.

Every other view of a trained model goes through the MLP.  This module exports the field as the asset NeRF toolchains use
for previews, viewers and fast probes (PlenOctrees / "baked" NeRF style): one dense voxel volume of density, view-dependent
radiance as real spherical harmonics, and optional attributes (albedo, normal), marched directly by ``pn_volume.hip`` with
empty-space skipping over 8^3-cell bricks.  Everything runs on the HIP device on the current stream (under
``torch.no_grad()`` except march_rays_ad); CPU tensors raise, there is no host fallback.

    RadianceVolume(data, bounds, sh_degree, attributes)   data [nx, ny, nz, C] on geometry's vertex grid
      .sigma / .coeff / .attributes             views: [nx, ny, nz], [nx, ny, nz, K, 3], name -> [nx, ny, nz, w]
      .occupancy / .refresh()                   one byte per brick (pn_volume_occupancy), built lazily; refresh after edits
      .save(path) / RadianceVolume.load(path, device)   volume.json + volume.bin, bit for bit
      .to_sparse(dtype)                         the occupied bricks only, as a SparseRadianceVolume
    SparseRadianceVolume(table, pool, bounds, resolution, sh_degree, attributes)   table int32 [nbx, nby, nbz] (slot or -1),
                                                pool [B, 9, 9, 9, C] fp32 or fp16: the present bricks, marched in place
      .from_dense(vol, dtype) / .to_dense()     pn_volume_pack / pn_volume_unpack; fp32 round-trips bit for bit on every
                                                vertex of a present brick, the rest is 0
      .nbytes / .dense_nbytes / .bricks / .dtype / .occupancy
      .save(path) / .load(path, device)         volume.json + table.bin + pool.bin; load_volume(path) takes either kind
    fibonacci_directions(D)                     the fp64 spherical Fibonacci set the bake evaluates the colour along
    sh_basis(directions, sh_degree)             numpy fp64 [D, K] in lighting's order and constants
    bake_volume(model, bounds, resolution, ...) density_grid pruned at sigma_min, SH fitted to query_field's rgb, attributes
    march_rays(vol, origins, directions, near, far, ...)   dict of rgb [R, 3], depth [R, 1], acc [R, 1], attributes [R, w]
    render_volume(vol, camera, c2w, ...)        dict of [1, C, H, W] images for any camera of cameras.py
    render_volume_path(vol, camera, poses, ...) dict kind -> frames (or PNG / EXR files), as views.render_path
    volume_probes(vol, positions, ...)          [P, 3, H, W] HDR probes with lighting.light_probes' pixel directions
    march_rays_grad(vol, rays.., grad_rgb, grad_acc, ...)   the reverse sweep: int64 sums [N, 1 + 3 K] of `quantum`, and a flag
    finish_grad(vol, sums, flag, quantum, clear)   the fp32 gradient [nx, ny, nz, C] of vol.data (NaN if the flag is set)
    march_rays_ad(vol, rays.., outputs)         march_rays as an autograd function: vol.data.requires_grad_() just works
    fit_volume(vol, images, camera, poses, steps, ...)   Adam on sigma and the coefficients against images, in place

The contract of the marcher is stated in include/panonerf_hip.h, section "radiance volume", and argued in DESIGN.md 6o.
Conventions, not measurements: D = 4 K baking directions, a marching step of half the smallest grid step, t_min = 1e-3 and
bricks of 8 cells.  sigma_min = 0.01 / |box diagonal| is derived: pruning removes at most 0.01 of optical depth from any
ray through the box.

The sparse form is stated in the header's section "sparse radiance volume" and argued in DESIGN.md 6p: marching it gives
the bits of marching its dense expansion, because the marcher's arithmetic is fp64 on the stored values either way.

The gradient of the marcher is stated in the header's section "radiance volume: gradients" and argued in DESIGN.md 6t: the
reverse sweep scatters 64-bit integers of a power-of-two quantum, so a gradient is the same bits whatever the order of
the rays.  fit_volume's two learning rates are conventions (profiles/volume_fit.txt has the sweep).

Out of scope: a split sigma / colour pool, quantised or block-compressed storage, hashed tables, bricks other than 8,
editing a sparse volume in place, an fp32-arithmetic marcher, cone-aware (mip) filtering, baking the surface / shading
branch, and stereo baking.  Of the gradients: sparse and fp16 gradients; depth, attribute, ray and camera gradients; TV or
sparsity regularisers; data-parallel fitting; growing or pruning the grid.
"""
import json
import math
import os

import numpy as np
import torch

from . import _lib, views
from .cameras import PanoCamera, _c2w_stack, _camera
from .geometry import _model_device, _placement, _resolution, _variance, density_grid, grid_points, query_field
from .rays import CameraRig, RayPool

BRICK = 8          # PN_VOLUME_BRICK
BRICK_VERTICES = (BRICK + 1) ** 3  # a stored brick: its 8^3 cells' vertices, the shared far faces included
_DENSE_FORMAT, _SPARSE_FORMAT = "pano_nerf_amd.radiance_volume", "pano_nerf_amd.sparse_radiance_volume"
MAX_ATTR = 8       # PN_VOLUME_MAX_ATTR
GOLDEN_ANGLE = 2.399963229728653  # PN_VOLUME_GOLDEN_ANGLE = pi (3 - sqrt 5)
_SH_C = (0.28209479177387814, 0.48860251190291992, 1.0925484305920792, 0.31539156525252005, 0.54627421529603959)
_BAKE_ATTRIBUTES = ("albedo", "normal")
_CORE = ("rgb", "depth", "acc")
_TAPS = "taps"  # march_rays' diagnostic output
_PATH_KINDS = {"ldr": ("rgb", "ldr"), "hdr": ("rgb", None), "depth": ("depth", "depth"), "albedo": ("albedo", "albedo"),
               "normal": ("normal", "normal")}


def fibonacci_directions(count):
    """fp64 [D, 3] unit directions of the spherical Fibonacci set: y_i = 1 - (2 i + 1) / D, r = sqrt(1 - y^2),
    phi = i GOLDEN_ANGLE, (r cos phi, y, r sin phi)."""
    D = int(count)
    if D < 1:
        raise ValueError(f"a direction set needs at least one direction; got {count!r}")
    i = np.arange(D, dtype=np.float64)
    y = 1.0 - (2.0 * i + 1.0) / D
    r = np.sqrt(1.0 - y * y)
    phi = i * GOLDEN_ANGLE
    return np.stack([r * np.cos(phi), y, r * np.sin(phi)], 1)


def sh_basis(directions, sh_degree):
    """numpy fp64 [.., K] real SH basis, K = (sh_degree + 1)^2, at directions [.., 3]: the first K entries of
    lighting._sh_basis, with the header's constants, written as the marcher evaluates them."""
    n = np.asarray(directions, dtype=np.float64)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    c0, c1, c2, c3, c4 = _SH_C
    cols = [np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c3 * (3.0 * (z * z) - 1.0),
            c2 * (x * z), c4 * (x * x - y * y)]
    return np.stack(cols[:_sh_count(sh_degree)], -1)


def _sh_count(sh_degree):
    if sh_degree not in (0, 1, 2) or isinstance(sh_degree, bool):
        raise ValueError(f"sh_degree must be 0, 1 or 2; got {sh_degree!r}")
    return (int(sh_degree) + 1) ** 2


def _attributes(attributes):
    """((name, width), ...) of names (width 3) or (name, width) pairs"""
    out = []
    for a in attributes:
        name, width = (a, 3) if isinstance(a, str) else (a[0], int(a[1]))
        if not isinstance(name, str) or name in _CORE or width < 1 or name in [n for n, _ in out]:
            raise ValueError(f"attributes must be distinct names other than {_CORE}, each with a positive width; got {a!r}")
        out.append((name, width))
    if sum(w for _, w in out) > MAX_ATTR:
        raise ValueError(f"a volume carries at most {MAX_ATTR} attribute channels; got {out}")
    return tuple(out)


def _channels(sh_degree, attrs=()):
    """1 + 3 K + E: sigma, K coefficient triples and the attribute channels"""
    return 1 + 3 * _sh_count(sh_degree) + sum(w for _, w in attrs)


def _bounds(bounds):
    b = tuple(tuple(float(v) for v in c) for c in bounds)
    if len(b) != 2 or len(b[0]) != 3 or len(b[1]) != 3:
        raise ValueError(f"bounds must be ((x0, y0, z0), (x1, y1, z1)); got {bounds!r}")
    return b


def _grid(bounds, res):
    lo, step = _placement(bounds, res)
    if not all(math.isfinite(s) and s > 0.0 for s in step) or not all(math.isfinite(v) for v in lo):
        raise ValueError(f"bounds must be finite with x0 < x1, y0 < y1, z0 < z1; got {bounds!r}")
    return lo, step


def _device_only(device, what):
    if device.type != "cuda":
        raise RuntimeError(f"pano_nerf_amd.volume runs on a HIP device only ({what} on {device}); there is no CPU fallback")


class _Header:
    """What both kinds of volume carry, checked in one place: sh_degree, the attributes (_attrs, attribute_names), the
    resolution, the bounds, the grid's lo / step and the channel count 1 + 3 K + E."""

    def __init__(self, bounds, resolution, sh_degree, attributes=()):
        self._attrs = _attributes(attributes)
        self.channels = _channels(sh_degree, self._attrs)
        self.sh_degree = int(sh_degree)
        self.attribute_names = tuple(n for n, _ in self._attrs)
        self.resolution = _resolution(resolution)
        self.bounds = _bounds(bounds)
        self.lo, self.step = _grid(self.bounds, self.resolution)


# ------------------------------------------------------------------------------------------------------------ files
def _write_header(path, fmt, h, mid, tail):
    """path/volume.json: the fields every volume has, with a format's own fields before (mid) and after (tail) lo / step.
    Two dicts only because the key order of the files is kept as it was: the sparse format has fields on both sides."""
    os.makedirs(path, exist_ok=True)
    meta = dict(format=fmt, version=1, bounds=[list(c) for c in h.bounds], resolution=list(h.resolution),
                sh_degree=h.sh_degree, attributes=[[n, w] for n, w in h._attrs], channels=h.channels, **mid, lo=list(h.lo),
                step=list(h.step), **tail)
    with open(os.path.join(path, "volume.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


def _read_meta(path):
    with open(os.path.join(path, "volume.json")) as fh:
        return json.load(fh)


def _read_header(path, fmt, what):
    """-> (the fields of path/volume.json, their _Header); a file of another format or version raises"""
    meta = _read_meta(path)
    if meta.get("format") != fmt or meta.get("version") != 1:
        raise ValueError(f"{path}: not {what} (format {meta.get('format')!r}, version {meta.get('version')!r})")
    return meta, _Header(meta["bounds"], meta["resolution"], meta["sh_degree"], [tuple(a) for a in meta["attributes"]])


def write_volume_files(path, data, bounds, sh_degree, attributes=()):
    """Write a host array data [nx, ny, nz, C] as path/volume.json + path/volume.bin (raw little-endian fp32)."""
    a = np.asarray(data)
    h = _Header(bounds, a.shape[:3], sh_degree, attributes) if a.ndim == 4 else None
    if h is None or a.dtype != np.float32 or a.shape[3] != h.channels:
        raise ValueError(f"data must be fp32 [nx, ny, nz, 1 + 3 K + E]; got {a.dtype} {a.shape}")
    _write_header(path, _DENSE_FORMAT, h, {}, dict(dtype="<f4", order="[nx, ny, nz, C], C fastest"))
    with open(os.path.join(path, "volume.bin"), "wb") as fh:
        fh.write(np.ascontiguousarray(a, dtype="<f4").tobytes())


def read_volume_files(path):
    """-> (data fp32 [nx, ny, nz, C] host array, bounds, sh_degree, attributes) of what write_volume_files wrote"""
    _, h = _read_header(path, _DENSE_FORMAT, "a radiance volume")
    res, C = h.resolution, h.channels
    raw = np.fromfile(os.path.join(path, "volume.bin"), dtype="<f4")
    if raw.size != res[0] * res[1] * res[2] * C:
        raise ValueError(f"{path}: volume.bin holds {raw.size} floats, the header asks for {res} x {C}")
    return raw.astype(np.float32, copy=False).reshape(*res, C), h.bounds, h.sh_degree, h._attrs


def _brick_counts(res):
    return tuple((n + BRICK - 2) // BRICK for n in res)


def _check_pool_size(B, C):
    if B * BRICK_VERTICES * C >= 1 << 40:
        raise ValueError(f"a pool of {B} bricks x {BRICK_VERTICES} vertices x {C} channels passes the 2^40 values the layout "
                         "allows")


def write_sparse_volume_files(path, table, pool, bounds, resolution, sh_degree, attributes=()):
    """Write host arrays table int32 [nbx, nby, nbz] and pool fp32 / fp16 [B, 9, 9, 9, C] as path/volume.json +
    path/table.bin (<i4) + path/pool.bin (<f4 or <f2): the layout of include/panonerf_hip.h, "sparse radiance volume"."""
    t, p = np.asarray(table), np.asarray(pool)
    h = _Header(bounds, resolution, sh_degree, attributes)
    res, C = h.resolution, h.channels
    if t.dtype != np.int32 or t.shape != _brick_counts(res):
        raise ValueError(f"table must be int32 {_brick_counts(res)} for resolution {res}; got {t.dtype} {t.shape}")
    if p.dtype not in (np.float32, np.float16) or p.ndim != 5 or p.shape[1:] != (BRICK + 1,) * 3 + (C,):
        raise ValueError(f"pool must be fp32 or fp16 [B, 9, 9, 9, 1 + 3 K + E = {C}]; got {p.dtype} {p.shape}")
    if int((t >= 0).sum()) != p.shape[0]:
        raise ValueError(f"table marks {int((t >= 0).sum())} bricks present, the pool holds {p.shape[0]}")
    dtype = "<f4" if p.dtype == np.float32 else "<f2"
    _write_header(path, _SPARSE_FORMAT, h, dict(bricks=int(p.shape[0]), dtype=dtype),
                  dict(brick=BRICK, order="table [nbx, nby, nbz] slot or -1; pool [B, 9, 9, 9, C], C fastest"))
    with open(os.path.join(path, "table.bin"), "wb") as fh:
        fh.write(np.ascontiguousarray(t, dtype="<i4").tobytes())
    with open(os.path.join(path, "pool.bin"), "wb") as fh:
        fh.write(np.ascontiguousarray(p, dtype=dtype).tobytes())


def read_sparse_volume_files(path):
    """-> (table int32 [nbx, nby, nbz], pool [B, 9, 9, 9, C] fp32 or fp16, bounds, resolution, sh_degree, attributes): host
    arrays of what write_sparse_volume_files wrote"""
    meta, h = _read_header(path, _SPARSE_FORMAT, "a sparse radiance volume")
    res, C = h.resolution, h.channels
    B = int(meta["bricks"])
    if meta.get("dtype") not in ("<f4", "<f2"):
        raise ValueError(f"{path}: the pool's dtype must be '<f4' or '<f2'; got {meta.get('dtype')!r}")
    nb = _brick_counts(res)
    table = np.fromfile(os.path.join(path, "table.bin"), dtype="<i4")
    if table.size != nb[0] * nb[1] * nb[2]:
        raise ValueError(f"{path}: table.bin holds {table.size} entries, resolution {res} has {nb} bricks")
    pool = np.fromfile(os.path.join(path, "pool.bin"), dtype=meta["dtype"])
    if B < 0 or pool.size != B * BRICK_VERTICES * C:
        raise ValueError(f"{path}: pool.bin holds {pool.size} values, the header asks for {B} x {BRICK_VERTICES} x {C}")
    dtype = np.float32 if meta["dtype"] == "<f4" else np.float16
    return (table.astype(np.int32, copy=False).reshape(nb), pool.astype(dtype, copy=False).reshape(B, *(BRICK + 1,) * 3, C),
            h.bounds, res, h.sh_degree, h._attrs)


def load_volume(path, device=None):
    """RadianceVolume.load or SparseRadianceVolume.load, by the `format` field of path/volume.json"""
    fmt = _read_meta(path).get("format")
    if fmt == _SPARSE_FORMAT:
        return SparseRadianceVolume.load(path, device)
    if fmt == _DENSE_FORMAT:
        return RadianceVolume.load(path, device)
    raise ValueError(f"{path}: not a radiance volume of either kind (format {fmt!r})")


def _load_device(device):
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    _device_only(dev, "a volume cannot be loaded")
    return dev


# ----------------------------------------------------------------------------------------------------------- volume
def _occupancy(res, C, data, dev):
    """uint8 [nbx, nby, nbz]: pn_volume_occupancy of channel 0 of a packed [nx, ny, nz, C] device tensor"""
    occ = torch.empty(_brick_counts(res), dtype=torch.uint8, device=dev)
    _lib.call("pn_volume_occupancy", *res, C, data.data_ptr(), occ.data_ptr(), _lib.stream(dev))
    return occ


class RadianceVolume(_Header):
    """One packed fp32 tensor data [nx, ny, nz, C] on the vertex grid of geometry.density_grid (bounds are the inclusive
    corner vertices, vertex (i ny + j) nz + k): channel 0 sigma, then K = (sh_degree + 1)^2 RGB coefficient triples in
    lighting's SH order, then the attribute channels.  `attributes`: names (width 3) or (name, width) pairs, e.g.
    (("albedo", 3), ("normal", 3)).  The tensor is held, not copied: edit it in place and call refresh()."""

    def __init__(self, data, bounds, sh_degree, attributes=()):
        if not isinstance(data, torch.Tensor) or data.dim() != 4:
            raise ValueError(f"data must be an [nx, ny, nz, C] tensor; got {getattr(data, 'shape', type(data))}")
        _device_only(data.device, "the data is")
        super().__init__(bounds, tuple(int(s) for s in data.shape[:3]), sh_degree, attributes)
        if data.shape[3] != self.channels:
            raise ValueError(f"data has {data.shape[3]} channels; sh_degree {sh_degree} with attributes {self._attrs} "
                             f"takes 1 + 3 K + E = {self.channels}")
        if data.dtype != torch.float32 or not data.is_contiguous():
            raise ValueError("data must be a contiguous fp32 tensor (it is held and read in place)")
        self.data = data.detach()
        self.device = data.device
        self._occ = None

    @property
    def sigma(self):
        return self.data[..., 0]

    @property
    def coeff(self):
        K = _sh_count(self.sh_degree)
        return self.data[..., 1:1 + 3 * K].unflatten(-1, (K, 3))

    @property
    def attributes(self):
        out, first = {}, _channels(self.sh_degree)
        for name, w in self._attrs:
            out[name] = self.data[..., first:first + w]
            first += w
        return out

    @property
    def occupancy(self):
        """uint8 [nbx, nby, nbz], one byte per brick of 8^3 cells: 1 iff a vertex of the brick has sigma > 0"""
        if self._occ is None:
            self.refresh()
        return self._occ

    def refresh(self):
        """Rebuild the occupancy from data (one launch of pn_volume_occupancy); call it after editing data.  Returns self."""
        with torch.no_grad(), torch.cuda.device(self.device):
            self._occ = _occupancy(self.resolution, self.channels, self.data, self.device)
        return self

    def save(self, path):
        """path/volume.json (bounds, resolution, sh_degree, attribute names and widths; lo / step for information) and
        path/volume.bin (the raw little-endian fp32 data)"""
        write_volume_files(path, self.data.cpu().numpy(), self.bounds, self.sh_degree, self._attrs)

    @classmethod
    def load(cls, path, device=None):
        dev = _load_device(device)
        data, bounds, sh_degree, attrs = read_volume_files(path)
        return cls(torch.from_numpy(np.ascontiguousarray(data)).to(dev), bounds, sh_degree, attrs)

    def to_sparse(self, dtype=torch.float32):
        """SparseRadianceVolume.from_dense(self, dtype): the occupied bricks only, in fp32 or fp16"""
        return SparseRadianceVolume.from_dense(self, dtype)


# ---------------------------------------------------------------------------------------------------- sparse volume
def _pool_dtype(dtype):
    if dtype not in (torch.float32, torch.float16):
        raise ValueError(f"a brick pool is torch.float32 or torch.float16; got {dtype!r}")
    return dtype


def _brick_table(occ):
    """(table int32 like occ, B): slots 0 .. B - 1 in ascending brick index, -1 where occ is 0 (one host sync for B)"""
    flat = occ.reshape(-1).to(torch.int64)
    slots = torch.cumsum(flat, 0) - flat  # exclusive
    table = torch.where(flat > 0, slots, -1).to(torch.int32).view(occ.shape)
    return table, int(flat.sum())


def _channel_name(ch, sh_degree, attrs):
    if ch == 0:
        return "sigma"
    first = _channels(sh_degree)  # the first attribute channel
    if ch < first:
        return f"coeff[{(ch - 1) // 3}][{'rgb'[(ch - 1) % 3]}]"
    ch -= first
    for name, w in attrs:
        if ch < w:
            return f"{name}[{ch}]"
        ch -= w
    return f"channel {ch}"


def _pack(res, C, table, B, dtype, dev, data=None, rows=None, vertex_row=None):
    """the pool [B, 9, 9, 9, C] of `table`, by pn_volume_pack from the dense data or from rows + vertex_row"""
    _check_pool_size(B, C)
    pool = torch.empty(B, BRICK + 1, BRICK + 1, BRICK + 1, C, dtype=dtype, device=dev)
    M = 0 if rows is None else int(rows.shape[0])
    _lib.call("pn_volume_pack", *res, C, table.data_ptr(), B, _lib.ptr(data), _lib.ptr(rows) if M else None, M,
              _lib.ptr(vertex_row), int(dtype == torch.float16), pool.data_ptr() if B else None, _lib.stream(dev))
    return pool


class SparseRadianceVolume(_Header):
    """The radiance volume with its unoccupied bricks left out: table int32 [nbx, nby, nbz] (a brick's slot in the pool,
    or -1; slots ascend with the brick index) and pool [B, 9, 9, 9, C] in fp32 or fp16, a present brick's 9^3 vertices
    with C fastest (include/panonerf_hip.h, "sparse radiance volume").  Made by RadianceVolume.to_sparse / from_dense or
    by bake_volume(sparse=True); marched in place by every function that takes a RadianceVolume.  Vertices on shared
    faces are stored once per present brick, so this is not a volume to edit in place: go through to_dense()."""

    def __init__(self, table, pool, bounds, resolution, sh_degree, attributes=()):
        super().__init__(bounds, resolution, sh_degree, attributes)
        for t, what in ((table, "table"), (pool, "pool")):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{what} must be a tensor; got {type(t).__name__}")
            _device_only(t.device, f"the {what} is")
        nb, C = _brick_counts(self.resolution), self.channels
        if table.dtype != torch.int32 or tuple(table.shape) != nb or not table.is_contiguous():
            raise ValueError(f"table must be a contiguous int32 {nb} tensor for resolution {self.resolution}; got "
                             f"{table.dtype} {tuple(table.shape)}")
        if pool.dim() != 5 or tuple(pool.shape[1:]) != (BRICK + 1,) * 3 + (C,):
            raise ValueError(f"pool must be [B, 9, 9, 9, C] with 1 + 3 K + E = {C} channels for sh_degree {sh_degree} and "
                             f"attributes {self._attrs}; got {tuple(pool.shape)}")
        if pool.dtype not in (torch.float32, torch.float16) or not pool.is_contiguous():
            raise ValueError("pool must be a contiguous fp32 or fp16 tensor (it is held and read in place)")
        if pool.device != table.device:
            raise ValueError(f"table is on {table.device} but pool on {pool.device}")
        B = int(pool.shape[0])
        _check_pool_size(B, C)
        # the marcher trusts the table: every entry is -1 or the next slot, and there are B of them (one host sync)
        flat = table.detach().reshape(-1)
        present = flat >= 0
        want = torch.where(present, torch.cumsum(present.to(torch.int64), 0) - 1, -1)
        if not bool(((flat == want).all()) & (present.sum() == B)):
            raise ValueError(f"table must hold -1 or the slots 0 .. {B - 1} of the pool in ascending brick index")
        self.table, self.pool = table.detach(), pool.detach()
        self.device = table.device

    @property
    def dtype(self):
        return self.pool.dtype

    @property
    def bricks(self):
        return int(self.pool.shape[0])

    @property
    def occupancy(self):
        """uint8 [nbx, nby, nbz]: 1 iff the brick is present"""
        return (self.table >= 0).to(torch.uint8)

    @property
    def nbytes(self):
        """bytes of the table and the pool"""
        return self.table.numel() * 4 + self.pool.numel() * self.pool.element_size()

    @property
    def dense_nbytes(self):
        """bytes of the dense fp32 tensor [nx, ny, nz, C] this volume expands to"""
        return self.resolution[0] * self.resolution[1] * self.resolution[2] * self.channels * 4

    @classmethod
    def from_dense(cls, vol, dtype=torch.float32):
        """Pack the occupied bricks of a RadianceVolume (its occupancy is rebuilt from the data first): occupancy, an
        exclusive prefix sum for the slots (one host sync for B), pn_volume_pack.  With fp16 a finite value of a present
        brick that rounds to an infinity raises ValueError naming its channel (one more sync)."""
        if not isinstance(vol, RadianceVolume):
            raise ValueError(f"from_dense takes a RadianceVolume; got {type(vol).__name__}")
        dtype = _pool_dtype(dtype)
        dev = vol.device
        with torch.no_grad(), torch.cuda.device(dev):
            table, B = _brick_table(vol.refresh().occupancy)
            pool = _pack(vol.resolution, vol.channels, table, B, dtype, dev, data=vol.data)
            out = cls(table, pool, vol.bounds, vol.resolution, vol.sh_degree, vol._attrs)
            if dtype == torch.float16 and bool(torch.isinf(pool).any()):
                # rare: tell the infinities the source had from the ones the rounding made
                bad = torch.isinf(out.to_dense().data) & torch.isfinite(vol.data)
                chans = torch.nonzero(bad.view(-1, vol.channels).any(0)).view(-1).tolist()
                if chans:
                    names = ", ".join(_channel_name(c, vol.sh_degree, vol._attrs) for c in chans)
                    raise ValueError(f"fp16 storage overflows in {names}: a finite value of a present brick has magnitude "
                                     ">= 65520")
        return out

    def to_dense(self):
        """The RadianceVolume this volume expands to (pn_volume_unpack): the stored value on every vertex of a present
        brick, fp16 widened exactly, and 0 elsewhere."""
        with torch.no_grad(), torch.cuda.device(self.device):
            data = torch.empty(*self.resolution, self.channels, dtype=torch.float32, device=self.device)
            _lib.call("pn_volume_unpack", *self.resolution, self.channels, self.table.data_ptr(), self.bricks,
                      self.pool.data_ptr() if self.bricks else None, int(self.dtype == torch.float16), data.data_ptr(),
                      _lib.stream(self.device))
        return RadianceVolume(data, self.bounds, self.sh_degree, self._attrs)

    def save(self, path):
        """path/volume.json, path/table.bin (<i4) and path/pool.bin (<f4 or <f2), by write_sparse_volume_files"""
        write_sparse_volume_files(path, self.table.cpu().numpy(), self.pool.cpu().numpy(), self.bounds, self.resolution,
                                  self.sh_degree, self._attrs)

    @classmethod
    def load(cls, path, device=None):
        dev = _load_device(device)
        table, pool, bounds, res, sh_degree, attrs = read_sparse_volume_files(path)
        return cls(torch.from_numpy(np.ascontiguousarray(table)).to(dev), torch.from_numpy(np.ascontiguousarray(pool)).to(dev),
                   bounds, res, sh_degree, attrs)


# ------------------------------------------------------------------------------------------------------------- bake
def bake_volume(model, bounds, resolution, sh_degree=1, directions=None, sigma_min=None, attributes=("albedo", "normal"),
                variance=None, chunk_rows=None, sparse=False, dtype=torch.float32):
    """Bake `model` into a RadianceVolume on the grid of density_grid(model, bounds, resolution, variance); with
    sparse=True into a SparseRadianceVolume of `dtype` (fp32 or fp16) whose to_dense() is that RadianceVolume bit for bit
    (fp32), without ever allocating the dense tensor: the survivors' rows [M, C] are evaluated by the same calls in the
    same order and packed into the present bricks through a vertex -> row map (pn_volume_pack).

    sigma is density_grid's, bit for bit, where it is > sigma_min and exactly 0 elsewhere (pruned; every channel of a pruned
    vertex is 0).  sigma_min None is 0.01 / |box diagonal|: trilinear interpolation is a convex combination, so pruning
    lowers the interpolated sigma by at most sigma_min anywhere, and no chord of the box is longer than its diagonal.
    sigma_min = 0 keeps everything positive.  Only the surviving vertices are evaluated further (one host synchronisation
    for their count): query_field(..., viewdirs=d_i, outputs=("rgb",)) along each of D directions at the grid's variance,
    and the coefficients are the least-squares fit P @ rgb, P = pinv(Y [D, K]) in fp64 on the host, applied in fp64 in
    direction order and rounded once.  directions: [D, 3] (numpy or tensor), None = fibonacci_directions(4 K), a convention;
    they are rounded to fp32 first, and Y is evaluated at what the field sees.  attributes: "albedo" (PanoMipNeRF only)
    and / or "normal", query_field's at the same rows, bit for bit."""
    K = _sh_count(sh_degree)
    if sparse:
        dtype = _pool_dtype(dtype)
    attributes = tuple(attributes)
    bad = [a for a in attributes if a not in _BAKE_ATTRIBUTES]
    if bad or len(set(attributes)) != len(attributes):
        raise ValueError(f"unknown attributes {bad or attributes}; choose from {_BAKE_ATTRIBUTES}")
    if "albedo" in attributes and model._NC != 5:
        raise ValueError(f"albedo needs a 5-channel density head (PanoMipNeRF); {type(model).__name__} has {model._NC}")
    res = _resolution(resolution)
    b = _bounds(bounds)
    _, step = _grid(b, res)
    if isinstance(variance, torch.Tensor):
        raise ValueError("bake_volume takes a scalar variance")
    variance = float(_variance(model, variance, step))
    if sigma_min is None:
        sigma_min = 0.01 / math.sqrt(sum((h - l) ** 2 for l, h in zip(*b)))
    sigma_min = float(sigma_min)
    if not sigma_min >= 0.0:
        raise ValueError(f"sigma_min must be >= 0; got {sigma_min!r}")
    if directions is None:
        dirs = fibonacci_directions(4 * K)
    else:
        dirs = directions.detach().cpu().numpy() if isinstance(directions, torch.Tensor) else np.asarray(directions)
        if dirs.ndim != 2 or dirs.shape[1] != 3 or dirs.shape[0] < K:
            raise ValueError(f"directions must be [D, 3] with D >= K = {K}; got {dirs.shape}")
    dirs32 = np.ascontiguousarray(dirs, dtype=np.float32)
    P = np.linalg.pinv(sh_basis(dirs32.astype(np.float64), sh_degree))  # [K, D]
    dev = _model_device(model)
    N = res[0] * res[1] * res[2]
    attrs = tuple((a, 3) for a in attributes)
    C = _channels(sh_degree, attrs)

    def fill(dst, sel, idx):
        """the survivors' channels into dst[sel]: the dense tensor at rows idx, or the compact rows themselves"""
        M = int(idx.shape[0])
        dst[sel, 0] = sigma[idx]
        pts = grid_points(b, res, 0.0, dev)[0][idx]
        dirs_t = torch.from_numpy(dirs32).to(dev)
        P_t = torch.from_numpy(P).to(dev)
        coef = torch.zeros(M, K, 3, dtype=torch.float64, device=dev)
        for i in range(dirs32.shape[0]):
            rgb = query_field(model, pts, variance, viewdirs=dirs_t[i], outputs=("rgb",), chunk_rows=chunk_rows)["rgb"]
            coef += P_t[:, i].view(1, K, 1) * rgb.to(torch.float64).view(M, 1, 3)
        dst[sel, 1:1 + 3 * K] = coef.to(torch.float32).view(M, 3 * K)
        if attributes:
            q = query_field(model, pts, variance, outputs=attributes, chunk_rows=chunk_rows)
            for j, name in enumerate(attributes):
                dst[sel, 1 + 3 * K + 3 * j:4 + 3 * K + 3 * j] = q[name]

    with torch.no_grad(), torch.cuda.device(dev):
        sigma = density_grid(model, b, res, variance, chunk_rows).view(-1)
        if not sparse:
            data = torch.zeros(N, C, dtype=torch.float32, device=dev)
            idx = torch.nonzero(sigma > sigma_min).reshape(-1)  # the one host sync: the survivors size everything below
            if int(idx.shape[0]):
                fill(data, idx, idx)
            return RadianceVolume(data.view(*res, -1), b, sh_degree, attrs)
        # sparse: the [N, C] tensor is never made.  The pruned sigma alone is a 1-channel volume whose occupancy is the
        # baked volume's (a survivor has sigma > 0, so every brick that holds one is present)
        keep = sigma > sigma_min
        idx = torch.nonzero(keep).reshape(-1)
        M = int(idx.shape[0])
        pruned = torch.where(keep, sigma, 0.0).contiguous()
        table, B = _brick_table(_occupancy(res, 1, pruned, dev))
        del pruned, keep
        rows = torch.zeros(M, C, dtype=torch.float32, device=dev)
        if M:
            fill(rows, slice(None), idx)
        if dtype == torch.float16:
            over = torch.isfinite(rows) & ~torch.isfinite(rows.to(torch.float16))
            chans = torch.nonzero(over.any(0)).view(-1).tolist()
            if chans:
                names = ", ".join(_channel_name(c, sh_degree, attrs) for c in chans)
                raise ValueError(f"fp16 storage overflows in {names}: a baked value has magnitude >= 65520")
        vertex_row = torch.full((N,), -1, dtype=torch.int32, device=dev)
        vertex_row[idx] = torch.arange(M, dtype=torch.int32, device=dev)
        pool = _pack(res, C, table, B, dtype, dev, rows=rows, vertex_row=vertex_row)
    return SparseRadianceVolume(table, pool, b, res, sh_degree, attrs)


# ------------------------------------------------------------------------------------------------------------ march
def default_step(vol):
    """half the smallest grid step, as the fp32 value the kernel takes: a convention"""
    return float(np.float32(0.5 * min(vol.step)))


def _rows(t, R, width, what, dev):
    if isinstance(t, torch.Tensor):
        _device_only(t.device, f"{what} is")
        if t.device != dev:
            raise ValueError(f"{what} is on {t.device} but the volume on {dev}")
        if t.numel() != R * width:
            raise ValueError(f"{what} must hold {R} rows of {width}; got {tuple(t.shape)}")
        return t.detach().to(torch.float32).reshape(R, width).contiguous()
    if width != 1:
        raise ValueError(f"{what} must be an [R, {width}] tensor; got {type(t).__name__}")
    return torch.full((R, 1), float(t), dtype=torch.float32, device=dev)


def _ray_rows(vol, origins, directions, near, far, step, t_min):
    """(R, origins [R, 3], directions [R, 3], near [R, 1], far [R, 1], step, t_min) as every marcher takes them: fp32 rows
    on the volume's device and the two march parameters as the fp32 values the kernel sees"""
    for t, what in ((origins, "origins"), (directions, "directions")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{what} must be an [R, 3] tensor; got {getattr(t, 'shape', type(t))}")
    step = default_step(vol) if step is None else float(np.float32(step))
    t_min = float(np.float32(t_min))
    if not (step > 0.0 and math.isfinite(step)) or not (t_min >= 0.0 and math.isfinite(t_min)):
        raise ValueError(f"step must be positive and finite and t_min >= 0; got {step!r}, {t_min!r}")
    dev, R = vol.device, int(origins.shape[0])
    return (R, _rows(origins, R, 3, "origins", dev), _rows(directions, R, 3, "directions", dev), _rows(near, R, 1, "near", dev),
            _rows(far, R, 1, "far", dev), step, t_min)


def march_rays(vol, origins, directions, near, far, step=None, t_min=1e-3, skip=True, outputs=("rgb", "depth", "acc")):
    """March rows of rays through `vol` in one launch of pn_volume_march (a RadianceVolume) or pn_volume_march_sparse (a
    SparseRadianceVolume, read in place): dict of rgb [R, 3], depth [R, 1], acc [R, 1] and one [R, w] per requested
    attribute name, fp32 on the volume's device.

    origins, directions: [R, 3] device tensors (directions need not be unit: t runs along them as given, as in Rays); near,
    far: floats or [R] / [R, 1] tensors.  step: the world distance between samples, None = half the smallest grid step (a
    convention); t_min: stop once the transmittance falls below it (0 never stops).  skip=True jumps over unoccupied
    bricks and gives the same bits as skip=False.  depth is the renderer's expected distance by its own rule
    (clamp(wt / acc, near, far), 0 / 0 -> 0), so it feeds warp_view, fusion and relight unchanged; there is no background
    term: callers have acc.  A diagnostic besides: "taps" [R, 2] int32, the samples whose sigma was interpolated and, of
    those, the ones that read the colour too (what tools/profile_volume.py counts the gathered bytes with)."""
    if not isinstance(vol, (RadianceVolume, SparseRadianceVolume)):
        raise ValueError(f"vol must be a RadianceVolume or a SparseRadianceVolume; got {type(vol).__name__}")
    outputs = tuple(outputs)
    bad = [o for o in outputs if o not in _CORE + vol.attribute_names + (_TAPS,)]
    if bad or not outputs:
        raise ValueError(f"outputs must be a non-empty subset of {_CORE + vol.attribute_names}; got {outputs!r}")
    dev = vol.device
    R, o, d, tn, tf, step, t_min = _ray_rows(vol, origins, directions, near, far, step, t_min)
    E = vol.channels - _channels(vol.sh_degree)
    want_attr = any(k in vol.attribute_names for k in outputs)
    with torch.no_grad(), torch.cuda.device(dev):
        new = lambda w: torch.empty(R, w, dtype=torch.float32, device=dev)
        rgb = new(3) if "rgb" in outputs else None
        depth = new(1) if "depth" in outputs else None
        acc = new(1) if "acc" in outputs else None
        attrs = new(E) if want_attr else None
        taps = torch.empty(R, 2, dtype=torch.int32, device=dev) if _TAPS in outputs else None
        if isinstance(vol, SparseRadianceVolume):  # marched in place: the table is the occupancy
            entry = "pn_volume_march_sparse"
            store = (vol.table.data_ptr(), vol.pool.data_ptr() if vol.bricks else None, int(vol.dtype == torch.float16),
                     int(bool(skip)))
        else:
            entry = "pn_volume_march"
            store = (vol.data.data_ptr(), _lib.ptr(vol.occupancy if skip else None))
        _lib.call(entry, R, *vol.resolution, vol.sh_degree, E, *store, *vol.lo,
                  *vol.step, o.data_ptr(), d.data_ptr(), tn.data_ptr(), tf.data_ptr(), step, t_min,
                  *[_lib.ptr(x) if R else None for x in (rgb, depth, acc, attrs, taps)], _lib.stream(dev))
    got = dict(rgb=rgb, depth=depth, acc=acc, taps=taps)
    first = 0
    for name, w in vol._attrs:
        if attrs is not None:
            got[name] = attrs[:, first:first + w]
        first += w
    return {k: got[k] for k in outputs}


# --------------------------------------------------------------------------------------------------------- wrappers
def _march_rig(vol, rig, first, count, near, far, step, t_min, skip, outputs):
    """march_rays over rows [first, first + count) of a rig; a fisheye writes 0 outside its image circle"""
    idx = torch.arange(first, first + count, dtype=torch.int64, device=vol.device)
    rays, _ = rig.sample(idx, near, far)
    got = march_rays(vol, rays.origins, rays.directions, rays.near, rays.far, step, t_min, skip, outputs)
    return views._in_circle(rig.camera, rays, got)


def render_volume(vol, camera, c2w, outputs=("rgb", "depth"), near=0.0, far=10.0, step=None, t_min=1e-3, skip=True):
    """One view of the volume -> dict of [1, C, H, W] fp32 tensors keyed as `outputs` ("rgb", "depth", "acc" and the volume's
    attribute names): march_rays on the rays CameraRig.sample gives the camera (what render_view renders), for a panorama,
    pinhole, cube-map, fisheye (0 outside the image circle) or stereo-panorama camera."""
    camera = _camera(camera)
    H, W = camera.h, camera.w
    with torch.no_grad(), torch.cuda.device(vol.device):
        rig = CameraRig(camera, _c2w_stack(c2w, single=True), vol.device)
        got = _march_rig(vol, rig, 0, H * W, near, far, step, t_min, skip, tuple(outputs))
    return {k: v.reshape(1, H, W, -1).permute(0, 3, 1, 2) for k, v in got.items()}


def render_volume_path(vol, camera, poses, kinds=("ldr", "depth"), near=0.0, far=10.0, step=None, t_min=1e-3, skip=True,
                       exposure=0.0, out_dir=None):
    """March every pose of poses ([n, 4, 4] or [n, 3, 4] c2ws) and turn the outputs into frames, as views.render_path does:
    dict kind -> uint8 [n, H, W, 3] device tensor, each frame to_frame of render_volume's output (ldr <- rgb, depth <- depth
    with near / far, albedo and normal <- the volume's attributes of those names); "hdr" is rgb itself as fp32
    [n, H, W, 3].  Rays are indexed over (frame, pixel), one march_rays call per group of frames.  With out_dir, frames go
    to out_dir/<kind>/<i:05d>.png (hdr/<i:05d>.exr) and the returned dict is empty."""
    camera = _camera(camera)
    kinds = tuple(kinds)
    bad = [k for k in kinds if k not in _PATH_KINDS or _PATH_KINDS[k][0] not in _CORE + vol.attribute_names]
    if bad or not kinds:
        have = [k for k, v in _PATH_KINDS.items() if v[0] in _CORE + vol.attribute_names]
        raise ValueError(f"kinds must be a non-empty subset of {have} for this volume; got {kinds!r}")
    outputs = tuple(dict.fromkeys(_PATH_KINDS[k][0] for k in kinds))
    c2ws = _c2w_stack(poses)
    dev = vol.device
    sink = views._FrameSink(kinds, c2ws.shape[0], camera.h, camera.w, dev, out_dir)
    with torch.no_grad(), torch.cuda.device(dev):
        rig = CameraRig(camera, c2ws, dev)
        views._put_groups(sink, lambda first, count: _march_rig(vol, rig, first, count, near, far, step, t_min, skip, outputs),
                          _PATH_KINDS, near, far, exposure)
    return sink.frames


def volume_probes(vol, positions, height=32, width=64, near=0.0, far=10.0, step=None, t_min=1e-3, skip=True):
    """HDR radiance [P, 3, H, W] seen from each of positions [P, 3]: the volume marched along the pixel directions of
    lighting.light_probes (an identity-rotation panorama camera at the position), all probes in one march_rays call.
    lighting.sh_project, irradiance, ibl.bake_ibl and emitters take the result as they take light_probes'."""
    P = views._probe_positions(positions)
    _device_only(positions.device, "the positions are")
    H, W = int(height), int(width)
    if H < 2 or W < 2:
        raise ValueError(f"a probe needs height and width >= 2; got {height} x {width}")
    dev = vol.device
    with torch.no_grad(), torch.cuda.device(dev):
        rig = views._probe_rig(positions, PanoCamera(H, W), dev)
        if P == 0:
            return torch.empty(0, 3, H, W, dtype=torch.float32, device=dev)
        rgb = _march_rig(vol, rig, 0, P * H * W, near, far, step, t_min, skip, ("rgb",))["rgb"]
    return rgb.view(P, H, W, 3).permute(0, 3, 1, 2)


# -------------------------------------------------------------------------------------------------------- gradients
QUANTUM = 2.0 ** -40  # the unit of the integer gradient sums: |sum| < 2^63 QUANTUM = 2^23, each contribution off by <= 2^-41
_ADAM = (0.9, 0.999, 1e-8)  # beta1, beta2, eps of fit_volume's update: torch.optim.Adam's defaults
# fit_volume's default rates, conventions chosen from the sweep of tools/profile_volume_fit.py (profiles/volume_fit.txt):
# sigma moves by about LR_SIGMA / |box diagonal| per step, a coefficient by about LR_COEFF
LR_SIGMA, LR_COEFF = 10.0, 0.01


def _quantum(quantum):
    q = float(quantum)
    if not (2.0 ** -60 <= q <= 1.0) or math.frexp(q)[0] != 0.5:
        raise ValueError(f"quantum must be a power of two in [2^-60, 1]; got {quantum!r}")
    return q


def _dense(vol, what):
    if isinstance(vol, SparseRadianceVolume):
        raise ValueError(f"{what} takes a dense RadianceVolume: a brick pool stores the vertices on shared faces once per "
                         "present brick, so its copies would each get part of the gradient and drift apart.  Fit the dense "
                         "volume (to_dense()), then to_sparse()")
    if not isinstance(vol, RadianceVolume):
        raise ValueError(f"{what} takes a RadianceVolume; got {type(vol).__name__}")
    return _channels(vol.sh_degree)


def march_rays_grad(vol, origins, directions, near, far, grad_rgb=None, grad_acc=None, step=None, t_min=1e-3, skip=True,
                    quantum=QUANTUM, sums=None, flag=None):
    """The reverse of march_rays for a dense RadianceVolume, one launch of pn_volume_march_bwd: with the upstream gradients
    grad_rgb [R, 3] and grad_acc [R] / [R, 1] of a scalar L (None counts as zeros), add dL/d(sigma) and dL/d(coefficients)
    into `sums`, int64 [N, 1 + 3 K] in units of `quantum` (N = nx ny nz vertices), and return (sums, flag).  sums / flag
    None allocate zeros; given ones are accumulated into.  flag int32 [1] becomes non-zero if a contribution was not
    finite or reached 2^52 quanta (it then added nothing).  The sums are integers, so they are the same bits for any
    order of the rows, any split of them over calls, and with or without skip; |sum| must stay below 2^63 quantum
    (2^23 at the default).  The rays, step, t_min and skip are march_rays'.  finish_grad turns the sums into fp32."""
    Cg = _dense(vol, "march_rays_grad")
    quantum = _quantum(quantum)
    dev = vol.device
    R, o, d, tn, tf, step, t_min = _ray_rows(vol, origins, directions, near, far, step, t_min)
    g_rgb = None if grad_rgb is None else _rows(grad_rgb, R, 3, "grad_rgb", dev)
    g_acc = None if grad_acc is None else _rows(grad_acc, R, 1, "grad_acc", dev)
    N = vol.resolution[0] * vol.resolution[1] * vol.resolution[2]
    E = vol.channels - Cg
    with torch.no_grad(), torch.cuda.device(dev):
        if sums is None:
            sums = torch.zeros(N, Cg, dtype=torch.int64, device=dev)
        if flag is None:
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _check_workspace(sums, flag, N, Cg, dev)
        _lib.call("pn_volume_march_bwd", R, *vol.resolution, vol.sh_degree, E, vol.data.data_ptr(),
                  _lib.ptr(vol.occupancy if skip else None), *vol.lo, *vol.step, o.data_ptr(), d.data_ptr(), tn.data_ptr(),
                  tf.data_ptr(), step, t_min, _lib.ptr(g_rgb) if R else None, _lib.ptr(g_acc) if R else None, quantum,
                  sums.data_ptr(), flag.data_ptr(), _lib.stream(dev))
    return sums, flag


def _check_workspace(sums, flag, N, Cg, dev):
    if (not isinstance(sums, torch.Tensor) or sums.dtype != torch.int64 or tuple(sums.shape) != (N, Cg)
            or not sums.is_contiguous() or sums.device != dev):
        raise ValueError(f"sums must be a contiguous int64 [{N}, {Cg}] tensor on {dev}; got "
                         f"{getattr(sums, 'dtype', type(sums))} {tuple(getattr(sums, 'shape', ()))}")
    if not isinstance(flag, torch.Tensor) or flag.dtype != torch.int32 or flag.numel() != 1 or flag.device != dev:
        raise ValueError(f"flag must be an int32 [1] tensor on {dev}")


def finish_grad(vol, sums, flag, quantum=QUANTUM, clear=False):
    """fp32 [nx, ny, nz, C], the gradient of march_rays_grad's scalar with respect to vol.data (pn_volume_grad_finish):
    float(sums quantum) in the sigma and coefficient channels, 0 in the attribute channels, and NaN everywhere if the flag
    is set: a poisoned backward, visible downstream without a host synchronisation here.  clear=True zeroes sums and the
    flag on the way, ready for the next step."""
    Cg = _dense(vol, "finish_grad")
    quantum = _quantum(quantum)
    dev = vol.device
    N = vol.resolution[0] * vol.resolution[1] * vol.resolution[2]
    _check_workspace(sums, flag, N, Cg, dev)
    with torch.no_grad(), torch.cuda.device(dev):
        grad = torch.empty(*vol.resolution, vol.channels, dtype=torch.float32, device=dev)
        _lib.call("pn_volume_grad_finish", N, vol.channels, Cg, sums.data_ptr(), quantum, flag.data_ptr(), grad.data_ptr(),
                  int(bool(clear)), _lib.stream(dev))
    return grad


class _MarchRaysAD(torch.autograd.Function):
    """march_rays with a gradient for vol.data: forward is march_rays (the same bits), backward march_rays_grad +
    finish_grad at the default quantum."""

    @staticmethod
    def forward(ctx, data, vol, origins, directions, near, far, step, t_min, skip, outputs):
        got = march_rays(vol, origins, directions, near, far, step, t_min, skip, outputs)
        ctx.save_for_backward(data)  # an in-place edit of the volume before backward() raises there
        ctx.vol, ctx.rays, ctx.params, ctx.outputs = vol, (origins, directions, near, far), (step, t_min, skip), outputs
        ctx.occ = vol.occupancy if skip else None  # the table this pass marched with
        flat = tuple(got[k] for k in outputs)
        ctx.mark_non_differentiable(*[t for k, t in zip(outputs, flat) if k not in ("rgb", "acc")])
        return flat

    @staticmethod
    def backward(ctx, *grads):
        (data,) = ctx.saved_tensors
        vol = ctx.vol
        if data.data_ptr() != vol.data.data_ptr():
            raise RuntimeError("the volume's data tensor was replaced between march_rays_ad and backward()")
        g = dict(zip(ctx.outputs, grads))
        step, t_min, skip = ctx.params
        occ, vol._occ = vol._occ, ctx.occ if skip else vol._occ
        try:
            sums, flag = march_rays_grad(vol, *ctx.rays, g.get("rgb"), g.get("acc"), step, t_min, skip)
        finally:
            vol._occ = occ
        return (finish_grad(vol, sums, flag),) + (None,) * 9


def march_rays_ad(vol, origins, directions, near, far, step=None, t_min=1e-3, skip=True, outputs=("rgb", "acc")):
    """march_rays as a torch.autograd.Function: the same dict of the same bits, with rgb and acc differentiable with respect
    to vol.data (only: rays and attributes get no gradient), so vol.data.requires_grad_() works with any torch loss and
    optimiser.  Dense volumes only.  The gradient is the one of march_rays_grad + finish_grad at the default quantum; it
    is all NaN if the flag was set.  vol.data is saved through save_for_backward, so an in-place edit between the two
    passes raises in backward(), and the backward marches with the occupancy table the forward used.  With
    vol.data.requires_grad, asking for depth or an attribute raises: they have no backward here."""
    _dense(vol, "march_rays_ad")
    outputs = tuple(outputs)
    if vol.data.requires_grad:
        bad = [k for k in outputs if k not in ("rgb", "acc")]
        if bad:
            raise ValueError(f"{bad} have no gradient: with vol.data.requires_grad, outputs must be a subset of "
                             "('rgb', 'acc')")
    flat = _MarchRaysAD.apply(vol.data, vol, origins, directions, near, far, step, t_min, skip, outputs)
    return dict(zip(outputs, flat))


def fit_volume(vol, images, camera, poses, steps, batch_rays=4096, lr_sigma=None, lr_coeff=None, loss=None, near=0.0,
               far=10.0, step=None, t_min=1e-3, seed=0, callback=None):
    """Fit a dense RadianceVolume, in place, to images [V, 3, H, W] (render_view's fine_rgb, render_volume's rgb or captured
    HDR frames: no model is needed) seen through `camera` at poses [V, 4, 4]: `steps` steps of Adam on batches of
    batch_rays pixels drawn by a rays.RayPool over CameraRig(camera, poses) with a generator seeded by `seed`.

    loss None is the mean squared error on rgb, whose gradient (pred - target) (2 / (3 B)) is written out; a callable
    loss(pred_rgb [B, 3], pred_acc [B, 1], target [B, 3]) -> scalar is differentiated by torch.  Each step: march_rays,
    the upstream gradients, march_rays_grad into one reused workspace, finish_grad(clear=True), then Adam (beta 0.9 /
    0.999, eps 1e-8, bias-corrected) in tensor ops with the rate lr_sigma / |box diagonal| for sigma (so lr_sigma is
    scale-free: optical depth per box diagonal) and lr_coeff for the coefficients; the attribute channels are not
    touched.  None: LR_SIGMA and LR_COEFF, conventions.  Then sigma.clamp_(min=0) and vol.refresh(): the occupancy depends
    on sigma > 0.  Nothing synchronises with the host per step; every 100 steps and at the end the overflow flags seen
    so far are read together with the step's loss, and a set flag raises.  callback(step, loss_value) is called at those
    checks.  Returns the list of the checked (step, loss) pairs.  A fitted volume no longer is bake_volume's bits, and
    the sigma_min bound on what pruning removed no longer describes it."""
    Cg = _dense(vol, "fit_volume")
    camera = _camera(camera)
    dev = vol.device
    steps = int(steps)
    B = int(batch_rays)
    if steps < 0 or B < 1:
        raise ValueError(f"steps must be >= 0 and batch_rays >= 1; got {steps!r}, {batch_rays!r}")
    c2ws = _c2w_stack(poses)
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or tuple(images.shape) != (c2ws.shape[0], 3, camera.h,
                                                                                          camera.w):
        raise ValueError(f"images must be a [{c2ws.shape[0]}, 3, {camera.h}, {camera.w}] tensor; got "
                         f"{tuple(getattr(images, 'shape', ()))}")
    diag = math.sqrt(sum((h - l) ** 2 for l, h in zip(*vol.bounds)))
    lr = torch.full((Cg,), LR_COEFF if lr_coeff is None else float(lr_coeff), dtype=torch.float32, device=dev)
    lr[0] = (LR_SIGMA if lr_sigma is None else float(lr_sigma)) / diag
    b1, b2, eps = _ADAM
    checks = []
    with torch.cuda.device(dev):
        with torch.no_grad():
            pool = RayPool(CameraRig(camera, c2ws, dev), images.detach().to(dev, torch.float32).permute(0, 2, 3, 1), near, far)
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))
            par = vol.data.view(-1, vol.channels)[:, :Cg]  # a view: sigma and the coefficients
            m, v = torch.zeros_like(par), torch.zeros_like(par)
            sums = torch.zeros(par.shape[0], Cg, dtype=torch.int64, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            seen = torch.zeros(1, dtype=torch.int32, device=dev)
        for it in range(1, steps + 1):
            with torch.no_grad():
                rays, target = pool.sample(B, gen)
                rows = (rays.origins, rays.directions, rays.near, rays.far)
                pred = march_rays(vol, *rows, step, t_min, True, ("rgb", "acc"))
            if loss is None:
                with torch.no_grad():
                    diff = pred["rgb"] - target
                    value = (diff * diff).mean()
                    g_rgb, g_acc = diff * (2.0 / (3 * B)), None
            else:
                p_rgb, p_acc = pred["rgb"].requires_grad_(), pred["acc"].requires_grad_()
                value = loss(p_rgb, p_acc, target)
                g_rgb, g_acc = torch.autograd.grad(value, (p_rgb, p_acc), allow_unused=True)
                value = value.detach()
            with torch.no_grad():
                march_rays_grad(vol, *rows, g_rgb, g_acc, step, t_min, True, QUANTUM, sums, flag)
                seen |= flag
                g = finish_grad(vol, sums, flag, QUANTUM, clear=True).view(-1, vol.channels)[:, :Cg]
                m = b1 * m + (1.0 - b1) * g
                v = b2 * v + (1.0 - b2) * (g * g)
                par.sub_(lr * ((m / (1.0 - b1 ** it)) / ((v / (1.0 - b2 ** it)).sqrt() + eps)))
                vol.sigma.clamp_(min=0)
                vol.refresh()
                if it % 100 == 0 or it == steps:
                    if int(seen):
                        raise RuntimeError(f"fit_volume: a gradient contribution was not finite or reached 2^52 quanta of "
                                           f"quantum = 2^-40 by step {it}; the volume now holds NaNs.  Scale the loss down")
                    checks.append((it, float(value)))
                    if callback is not None:
                        callback(it, checks[-1][1])
    return checks
