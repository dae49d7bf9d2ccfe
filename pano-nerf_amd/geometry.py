"""Export of the learned geometry: field queries, sigma volumes, marching-tetrahedra meshes and PLY files.

Everything runs on the HIP device through the kernels of ``libpanonerf_hip.so`` (``pn_geometry.hip`` plus the MLP
entry points the renderer uses), under ``torch.no_grad()`` on the current stream.  CPU tensors raise: there is no host
fallback.  The only host synchronisation is the copy of the two mesh totals that sizes the outputs.

    query_field(model, points, ...)             sigma / albedo / rgb / normal / grad (d sigma / d mean) at [M, 3] points
    grid_points(bounds, resolution, ...)        the (mean, cov) rows of a grid's vertices
    density_grid(model, bounds, resolution)     sigma on an [nx, ny, nz] vertex grid
    marching_tetrahedra(sigma, level, bounds)   (vertices [V, 3], faces [F, 3] int32) of {sigma > level}
    extract_mesh(model, bounds, resolution, level)  Mesh(vertices, faces, normals, colors)
    write_ply(path, vertices, faces, normals, colors)  binary little-endian PLY
    read_ply(path)                              Mesh of host numpy arrays from such a file (binary or ASCII)
    read_obj(path)                              ObjMesh of host numpy arrays from a Wavefront OBJ (+ MTL) file

The mesh contract (edge ids, vertex and face order, winding) is stated in include/panonerf_hip.h.
"""
import collections
import os

import numpy as np
import torch

from . import _lib
from .render import _Field

Mesh = collections.namedtuple("Mesh", ["vertices", "faces", "normals", "colors"])
ObjMesh = collections.namedtuple("ObjMesh", ["vertices", "faces", "uv", "face_uv", "normals", "face_material", "materials"])

FIELD_OUTPUTS = ("sigma", "albedo", "rgb", "normal", "grad")

# default rows per chunk: the layer-wise path keeps ~10 KB per row (activations), +8 KB for the density-gradient sweep;
# the chains keep ~0.7 KB (gate words, encoding, raw outputs), +1 KB for the density-gradient slot
_CHUNK_LAYERWISE = 1 << 16
_CHUNK_CHAIN = 1 << 19


def _device_of(*tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.device.type != "cuda":
            raise RuntimeError("pano_nerf_amd.geometry runs on a HIP device only (a tensor is on %s); there is no CPU "
                               "fallback" % t.device)
    return tensors[0].device


def _model_device(model):
    dev = model.mlp.flat_params().device
    if dev.type != "cuda":
        raise RuntimeError("pano_nerf_amd.geometry runs on a HIP device only (the model is on %s); there is no CPU "
                           "fallback" % dev)
    return dev


def _resolution(resolution):
    r = (int(resolution),) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(x) for x in resolution)
    if len(r) != 3 or min(r) < 2:
        raise ValueError(f"resolution must be an int or 3 ints, each >= 2; got {resolution!r}")
    if r[0] * r[1] * r[2] >= 1 << 31:
        raise ValueError(f"resolution {r} has 2^31 or more vertices")
    return r


def _placement(bounds, res):
    """((x0, y0, z0), (dx, dy, dz)) of inclusive corner vertices `bounds` on `res` vertices per axis."""
    try:
        lo, hi = [tuple(float(v) for v in c) for c in bounds]
    except (TypeError, ValueError):
        raise ValueError(f"bounds must be ((x0, y0, z0), (x1, y1, z1)); got {bounds!r}")
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError(f"bounds must be ((x0, y0, z0), (x1, y1, z1)); got {bounds!r}")
    step = tuple((b - a) / (n - 1) for a, b, n in zip(lo, hi, res))
    # the kernels see fp32 values: report the same
    return tuple(float(np.float32(v)) for v in lo), tuple(float(np.float32(v)) for v in step)


def _variance(model, variance, step=None):
    if getattr(model, "disable_integration", False):  # models/pano_mip_nerf.py:241-243: zero covariance everywhere
        return 0.0
    if variance is None:
        return 0.0 if step is None else max(abs(s) for s in step) ** 2 / 12.0
    return variance


def _field_rows(model, dev, M, fill, outputs, viewdirs, chunk_rows, results):
    """Evaluate the field over M rows in chunks; fill(first, m, mean, cov) writes a chunk's (mean, cov) rows; results:
    output name -> [M, ...] tensor (or, for "sigma", any [M] view, e.g. a flat volume)."""
    f = _Field.of(model, dev)
    want_grad = "normal" in results or "grad" in results
    chunk = int(chunk_rows) if chunk_rows else (_CHUNK_CHAIN if f.planes else _CHUNK_LAYERWISE)
    if chunk <= 0:
        raise ValueError(f"chunk_rows must be positive; got {chunk_rows!r}")
    dummy_view = torch.zeros(1, 3, dtype=torch.float32, device=dev)
    for first in range(0, M, chunk):
        m = min(chunk, M - first)
        if viewdirs is None:  # sigma / albedo / normals do not read the view: one dummy view row for the whole chunk
            vd, rpr = dummy_view, m
        elif viewdirs.shape[0] == 1:
            vd, rpr = viewdirs, m
        else:
            vd, rpr = viewdirs[first:first + m], 1
        ev = f.evaluation(m, rpr, vd, False)
        fill(first, m, ev.mean, ev.cov)
        f.forward(ev)
        sl = lambda k: (results[k][first:first + m] if k in results else None)
        gmean = f.density_grad(ev, False, sl("grad")) if want_grad else None
        _lib.call("pn_field_epilogue", m, f.nc, f.density_bias, f.rgb_padding, ev.raw_rgb.data_ptr(),
                  ev.raw_den.data_ptr(), _lib.ptr(gmean), _lib.ptr(sl("sigma")), _lib.ptr(sl("albedo")),
                  _lib.ptr(sl("rgb")), _lib.ptr(sl("normal")), f.st)
        del ev


def _check_outputs(model, outputs, viewdirs):
    outputs = tuple(outputs)
    bad = [o for o in outputs if o not in FIELD_OUTPUTS]
    if bad:
        raise ValueError(f"unknown field outputs {bad}; choose from {FIELD_OUTPUTS}")
    if "albedo" in outputs and model._NC != 5:
        raise ValueError(f"albedo needs a 5-channel density head (PanoMipNeRF); {type(model).__name__} has {model._NC}")
    if "rgb" in outputs and viewdirs is None:
        raise ValueError("rgb needs viewdirs ([M, 3] or one [3] direction)")
    return outputs


def query_field(model, points, variance=None, viewdirs=None, outputs=("sigma", "albedo", "normal"), chunk_rows=None):
    """The trained field at `points` [M, 3]: a dict of [M] ("sigma") and [M, 3] ("albedo", "rgb", "normal" = -grad
    normalised, "grad" = d sigma / d mean) fp32 tensors on the points' device.

    variance: None (0: plain positional encoding), a float or an [M, 3] tensor - the diagonal covariance of the
    integrated encoding; a model built with disable_integration=True always uses 0.  viewdirs ([M, 3] or [3]) is needed
    for "rgb" only.  "albedo" needs a PanoMipNeRF (5 density channels).  chunk_rows bounds the rows evaluated at once."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be an [M, 3] tensor; got {getattr(points, 'shape', type(points))}")
    outputs = _check_outputs(model, outputs, viewdirs)
    if viewdirs is not None:
        if not isinstance(viewdirs, torch.Tensor) or viewdirs.shape not in ((3,), (points.shape[0], 3)):
            raise ValueError(f"viewdirs must be [M, 3] or [3]; got {getattr(viewdirs, 'shape', type(viewdirs))}")
    var_t = None
    if isinstance(variance, torch.Tensor):
        if variance.shape != points.shape:
            raise ValueError(f"a variance tensor must be [M, 3] like the points; got {tuple(variance.shape)}")
        var_t = variance
    dev = _device_of(points, *[t for t in (viewdirs, var_t) if t is not None])
    if _model_device(model) != dev:
        raise RuntimeError(f"points are on {dev}, the model on {_model_device(model)}")
    variance = _variance(model, variance)
    M = points.shape[0]
    with torch.no_grad(), torch.cuda.device(dev):
        pts = points.detach().to(torch.float32).contiguous()
        vd = None
        if viewdirs is not None:
            vd = viewdirs.detach().to(torch.float32).reshape(-1, 3).contiguous()
        cov_src = variance.detach().to(torch.float32).contiguous() if isinstance(variance, torch.Tensor) else None

        def fill(first, m, mean, cov):
            mean.copy_(pts[first:first + m])
            if cov_src is not None:
                cov.copy_(cov_src[first:first + m])
            else:
                cov.fill_(float(variance))

        res = {k: torch.empty((M,) if k == "sigma" else (M, 3), dtype=torch.float32, device=dev) for k in outputs}
        if M:
            _field_rows(model, dev, M, fill, outputs, vd if "rgb" in outputs else None, chunk_rows, res)
    return res


def grid_points(bounds, resolution, variance=0.0, device=None):
    """(mean, cov) [nx ny nz, 3] of the grid's vertices in vertex order (i ny + j) nz + k, as the kernels place them."""
    res = _resolution(resolution)
    lo, step = _placement(bounds, res)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("pano_nerf_amd.geometry runs on a HIP device only; there is no CPU fallback")
    n = res[0] * res[1] * res[2]
    with torch.cuda.device(dev):
        mean = torch.empty(n, 3, dtype=torch.float32, device=dev)
        cov = torch.empty(n, 3, dtype=torch.float32, device=dev)
        _lib.call("pn_grid_points", *res, 0, n, *lo, *step, float(variance), mean.data_ptr(), cov.data_ptr(),
                  _lib.stream(dev))
    return mean, cov


def density_grid(model, bounds, resolution, variance=None, chunk_rows=None):
    """sigma at the vertices of a grid: a contiguous fp32 [nx, ny, nz] tensor on the model's device.

    bounds = ((x0, y0, z0), (x1, y1, z1)) are the inclusive corner vertices; resolution is an int or 3 ints (vertices
    per axis, each >= 2).  variance: a float; None gives max(dx, dy, dz)^2 / 12, the second moment of a voxel."""
    res = _resolution(resolution)
    lo, step = _placement(bounds, res)
    if isinstance(variance, torch.Tensor):
        raise ValueError("density_grid takes a scalar variance")
    variance = float(_variance(model, variance, step))
    dev = _model_device(model)
    vol = torch.empty(res, dtype=torch.float32, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        st = _lib.stream(dev)

        def fill(first, m, mean, cov):
            _lib.call("pn_grid_points", *res, first, m, *lo, *step, variance, mean.data_ptr(), cov.data_ptr(), st)

        _field_rows(model, dev, vol.numel(), fill, ("sigma",), None, chunk_rows, {"sigma": vol.view(-1)})
    return vol


def marching_tetrahedra(sigma, level, bounds=None):
    """Iso-surface {sigma > level} of an [nx, ny, nz] volume: (vertices [V, 3] fp32, faces [F, 3] int32) on its device.

    Without bounds the vertices are in grid units from the origin (vertex (i, j, k) at (i, j, k)); with bounds, in the
    placement of density_grid.  Faces are wound so that (v1 - v0) x (v2 - v0) points to the outside (sigma <= level).
    An empty surface gives [0, 3] tensors."""
    if not isinstance(sigma, torch.Tensor) or sigma.dim() != 3:
        raise ValueError(f"sigma must be an [nx, ny, nz] tensor; got {getattr(sigma, 'shape', type(sigma))}")
    res = tuple(int(x) for x in sigma.shape)
    if min(res) < 2:
        raise ValueError(f"every axis of sigma must have >= 2 vertices; got {res}")
    if res[0] * res[1] * res[2] >= 1 << 31:
        raise ValueError(f"sigma {res} has 2^31 or more vertices")
    dev = _device_of(sigma)
    if bounds is None:
        lo, step = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    else:
        lo, step = _placement(bounds, res)
    level = float(level)
    with torch.no_grad(), torch.cuda.device(dev):
        st = _lib.stream(dev)
        s = sigma.detach().to(torch.float32).contiguous()
        work = torch.empty(int(_lib.load().pn_mt_work_bytes(*res)), dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.call("pn_mt_count", *res, s.data_ptr(), level, work.data_ptr(), totals.data_ptr(), st)
        nv, nf = (int(x) for x in totals.cpu())  # the one host sync: sizes the outputs
        if nv >= 1 << 31 or nf >= 1 << 31:
            raise RuntimeError(f"mesh of {nv} vertices / {nf} faces does not fit int32 indices; use a coarser grid")
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        _lib.call("pn_mt_emit", *res, s.data_ptr(), level, work.data_ptr(), nv, nf, *lo, *step,
                  _lib.ptr(verts) if nv else None, _lib.ptr(faces) if nf else None, st)
    return verts, faces


def extract_mesh(model, bounds, resolution, level, variance=None, normals=True, colors="auto", chunk_rows=None):
    """Mesh(vertices [V, 3], faces [F, 3] int32, normals [V, 3] | None, colors [V, 3] | None) of {sigma > level} on the
    model's device: density_grid -> marching_tetrahedra, then the field queried at the vertices with the grid's
    variance.  normals: the model's normals (-grad sigma, normalised).  colors: "auto" (albedo for PanoMipNeRF, radiance
    for MipNeRF), "albedo", "radiance" (rgb seen along -normal) or None."""
    if colors not in ("auto", "albedo", "radiance", None):
        raise ValueError(f"colors must be 'auto', 'albedo', 'radiance' or None; got {colors!r}")
    if colors == "auto":
        colors = "albedo" if model._NC == 5 else "radiance"
    if colors == "albedo" and model._NC != 5:
        raise ValueError(f"colors='albedo' needs a PanoMipNeRF (5 density channels); {type(model).__name__} has none")
    if level is None:
        raise ValueError("level is required")
    res = _resolution(resolution)
    _, step = _placement(bounds, res)
    if isinstance(variance, torch.Tensor):
        raise ValueError("extract_mesh takes a scalar variance")
    variance = float(_variance(model, variance, step))
    _model_device(model)
    sigma = density_grid(model, bounds, res, variance, chunk_rows)
    verts, faces = marching_tetrahedra(sigma, level, bounds)
    del sigma
    nrm = col = None
    want = (("normal",) if (normals or colors == "radiance") else ()) + (("albedo",) if colors == "albedo" else ())
    if want:
        q = query_field(model, verts, variance, outputs=want, chunk_rows=chunk_rows)
        nrm, col = q.get("normal"), q.get("albedo")
        if colors == "radiance":
            col = query_field(model, verts, variance, viewdirs=-nrm, outputs=("rgb",), chunk_rows=chunk_rows)["rgb"]
        if not normals:
            nrm = None
    return Mesh(verts, faces, nrm, col)


def write_ply(path, vertices, faces, normals=None, colors=None):
    """Binary little-endian PLY: float x y z [nx ny nz] [uchar red green blue] per vertex, a uchar-counted int list of
    vertex_indices per face.  Colours are clamped to [0, 1] and scaled by 255 (rounded to nearest)."""
    v = _host(vertices, np.float32, "vertices")
    f = _host(faces, np.int32, "faces")
    n = None if normals is None else _host(normals, np.float32, "normals")
    c = None if colors is None else _host(colors, np.float32, "colors")
    for name, a in (("normals", n), ("colors", c)):
        if a is not None and a.shape != v.shape:
            raise ValueError(f"{name} must be [V, 3] like the vertices; got {a.shape}")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if n is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if c is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vrec = np.empty(v.shape[0], dtype=fields)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if n is not None:
        vrec["nx"], vrec["ny"], vrec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if c is not None:
        q = np.rint(np.clip(np.nan_to_num(c), 0.0, 1.0) * 255.0).astype(np.uint8)
        vrec["red"], vrec["green"], vrec["blue"] = q[:, 0], q[:, 1], q[:, 2]
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"] = 3
    frec["i"] = f
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    head += [f"property float {k}" for k in ("x", "y", "z")]
    if n is not None:
        head += [f"property float {k}" for k in ("nx", "ny", "nz")]
    if c is not None:
        head += [f"property uchar {k}" for k in ("red", "green", "blue")]
    head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def _host(x, dtype, name):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{name} must be [N, 3]; got {a.shape}")
    return np.ascontiguousarray(a, dtype=dtype)


_PLY_VERTEX = {"x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"}


def read_ply(path):
    """Mesh(vertices [V, 3] fp32, faces [F, 3] int32, normals [V, 3] fp32 | None, colors [V, 3] fp32 in [0, 1] | None) as
    HOST numpy arrays (a file is host data; write_ply and objects.VirtualObject take them as they are and copy them to the
    device themselves).  Reads what write_ply writes - binary little-endian, float x y z, optional float nx ny nz,
    optional uchar red green blue, uchar-counted int (or uint) lists of 3 vertex_indices - and the ASCII form of the
    same elements.  Anything else raises ValueError naming what it found."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file (no 'ply' ... 'end_header' header)")
    nl = data.find(b"\n", end)
    if nl < 0:
        raise ValueError(f"{path}: the header's last line is not terminated")
    body = data[nl + 1:]
    fmt, elements = None, []  # elements: [name, count, [(kind, type(s), name)]]
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1] if len(w) > 1 else ""
        elif w[0] == "element" and len(w) == 3:
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property" and elements:
            if w[1] == "list" and len(w) == 5:
                elements[-1][2].append(("list", (w[2], w[3]), w[4]))
            elif len(w) == 3:
                elements[-1][2].append(("scalar", w[1], w[2]))
            else:
                raise ValueError(f"{path}: unreadable header line {line!r}")
        else:
            raise ValueError(f"{path}: unreadable header line {line!r}")
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError(f"{path}: format {fmt!r} is not supported (binary_little_endian or ascii)")
    if [e[0] for e in elements] != ["vertex", "face"]:
        raise ValueError(f"{path}: elements {[e[0] for e in elements]} (expected vertex, then face)")
    (_, nv, vprops), (_, nf, fprops) = elements
    names = [p[2] for p in vprops]
    for kind, typ, name in vprops:
        want = ("uchar", "uint8") if name in ("red", "green", "blue") else ("float", "float32")
        if kind != "scalar" or name not in _PLY_VERTEX or typ not in want:
            raise ValueError(f"{path}: vertex property {typ if kind == 'scalar' else 'list'} {name} is not supported")
    groups = [g for g in (("x", "y", "z"), ("nx", "ny", "nz"), ("red", "green", "blue")) if any(k in names for k in g)]
    if names != [k for g in groups for k in g] or groups[:1] != [("x", "y", "z")]:
        raise ValueError(f"{path}: vertex properties {names} (expected x y z [nx ny nz] [red green blue])")
    if len(fprops) != 1 or fprops[0][0] != "list" or fprops[0][1][0] not in ("uchar", "uint8") or \
            fprops[0][1][1] not in ("int", "int32", "uint", "uint32") or fprops[0][2] not in ("vertex_indices", "vertex_index"):
        raise ValueError(f"{path}: face properties {fprops} (expected 'list uchar int vertex_indices')")
    has_n, has_c = "nx" in names, "red" in names
    if fmt == "ascii":
        tok = body.split()
        ncol = len(names)
        if len(tok) < nv * ncol + nf * 4:
            raise ValueError(f"{path}: the body ends early")
        vt = np.array(tok[:nv * ncol], dtype=np.float64).reshape(nv, ncol)
        ft = np.array(tok[nv * ncol:nv * ncol + nf * 4], dtype=np.int64).reshape(nf, 4)
        if nf and not (ft[:, 0] == 3).all():
            raise ValueError(f"{path}: a face with {int(ft[ft[:, 0] != 3][0, 0])} vertices (only triangles are supported)")
        v = vt[:, :3].astype(np.float32)
        n = vt[:, 3:6].astype(np.float32) if has_n else None
        c = (vt[:, ncol - 3:] / 255.0).astype(np.float32) if has_c else None
        f = ft[:, 1:].astype(np.int32)
    else:
        fields = [(k, "u1" if k in ("red", "green", "blue") else "<f4") for k in names]
        vdt = np.dtype(fields)
        fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
        if len(body) < nv * vdt.itemsize:
            raise ValueError(f"{path}: the body ends early")
        vrec = np.frombuffer(body, dtype=vdt, count=nv)
        rest = body[nv * vdt.itemsize:]
        if nf and rest[0] != 3:
            raise ValueError(f"{path}: a face with {rest[0]} vertices (only triangles are supported)")
        if len(rest) < nf * fdt.itemsize:
            raise ValueError(f"{path}: the body ends early")
        frec = np.frombuffer(rest, dtype=fdt, count=nf)
        if nf and not (frec["n"] == 3).all():
            raise ValueError(f"{path}: a face with {int(frec['n'][frec['n'] != 3][0])} vertices (only triangles are supported)")
        v = np.stack([vrec["x"], vrec["y"], vrec["z"]], 1).astype(np.float32)
        n = np.stack([vrec["nx"], vrec["ny"], vrec["nz"]], 1).astype(np.float32) if has_n else None
        c = (np.stack([vrec["red"], vrec["green"], vrec["blue"]], 1).astype(np.float32) / np.float32(255.0)) if has_c else None
        f = np.ascontiguousarray(frec["i"], dtype=np.int32)
    return Mesh(v.reshape(nv, 3), f.reshape(nf, 3), n, c)


_MTL_MAPS = {"map_kd": "map_Kd", "map_pr": "map_Pr", "norm": "norm", "map_bump": "norm", "bump": "norm"}
_MTL_OPTIONS = {"-blendu": 1, "-blendv": 1, "-boost": 1, "-bm": 1, "-cc": 1, "-clamp": 1, "-imfchan": 1, "-texres": 1,
                "-type": 1, "-mm": 2, "-o": 3, "-s": 3, "-t": 3}


def _map_name(words):
    """the file name of an MTL map statement: options (and their arguments) before it are skipped"""
    i = 0
    while i < len(words) and words[i] in _MTL_OPTIONS:
        i += 1 + _MTL_OPTIONS[words[i]]
    if i >= len(words):
        raise ValueError(f"no file name in map statement {' '.join(words)!r}")
    return " ".join(words[i:])


def read_mtl(path):
    """Ordered dict name -> dict(Kd=(r, g, b) | None, Pr=float | None, map_Kd, map_Pr, norm = path | None) of an MTL
    file; norm is what `norm`, `map_Bump` or `bump` names.  Map paths are made relative to the MTL file's directory.
    Other keys are ignored."""
    base = os.path.dirname(os.path.abspath(path))
    mats, cur = collections.OrderedDict(), None
    with open(path, "r", errors="replace") as fh:
        for ln, line in enumerate(fh, 1):
            w = line.split("#", 1)[0].split()
            if not w:
                continue
            key = w[0]
            if key == "newmtl":
                if len(w) < 2:
                    raise ValueError(f"{path}:{ln}: newmtl without a name")
                cur = dict(Kd=None, Pr=None, map_Kd=None, map_Pr=None, norm=None)
                mats[" ".join(w[1:])] = cur
                continue
            if cur is None:
                continue
            try:
                if key == "Kd":
                    k = [float(x) for x in w[1:4]]
                    cur["Kd"] = tuple(k * 3 if len(k) == 1 else k)
                    if len(cur["Kd"]) != 3:
                        raise ValueError("Kd takes 1 or 3 values")
                elif key == "Pr":
                    cur["Pr"] = float(w[1])
                elif key.lower() in _MTL_MAPS:
                    cur[_MTL_MAPS[key.lower()]] = os.path.join(base, _map_name(w[1:]).replace("\\", "/"))
            except (ValueError, IndexError) as e:
                raise ValueError(f"{path}:{ln}: unreadable line {line.strip()!r} ({e})") from None
    return mats


def read_obj(path):
    """ObjMesh(vertices [V, 3] fp32, faces [F, 3] int32, uv [T, 2] fp32 | None, face_uv [F, 3] int32 | None, normals [V, 3]
    fp32, face_material [F] int32, materials) of a Wavefront OBJ file, as HOST numpy arrays.

    Read: v, vt, vn, f (corners `v`, `v/vt`, `v//vn`, `v/vt/vn`; 1-based or negative = relative to the end so far; polygons
    are fan-triangulated around their first corner), mtllib and usemtl.  Everything else (o, g, s, l, ...) is ignored.
    uv / face_uv are None unless every corner has a vt.  normals: the file's vn when every corner's vn index equals its
    v index (and there are as many vn as v); otherwise area-weighted vertex normals (the sum of e1 x e2 over a vertex's
    faces, normalised; 0 for a vertex no face uses).  materials: the ordered dict of read_mtl over every mtllib, plus an
    entry (all None) for a usemtl name no library defines; face_material indexes it, -1 for faces before any usemtl.  A
    mtllib file that does not exist raises FileNotFoundError naming it."""
    base = os.path.dirname(os.path.abspath(path))
    v, vt, vn = [], [], []
    fv, ft, fn, fm = [], [], [], []
    materials, cur = collections.OrderedDict(), -1

    def index(tok, n, what, ln):
        i = int(tok)
        j = i - 1 if i > 0 else n + i
        if i == 0 or not 0 <= j < n:
            raise ValueError(f"{path}:{ln}: {what} index {i} outside the {n} read so far")
        return j

    with open(path, "r", errors="replace") as fh:
        for ln, line in enumerate(fh, 1):
            w = line.split("#", 1)[0].split()
            if not w:
                continue
            key = w[0]
            try:
                if key == "v":
                    v.append([float(x) for x in w[1:4]])
                    if len(v[-1]) != 3:
                        raise ValueError("v takes 3 coordinates")
                elif key == "vt":
                    vt.append([float(x) for x in w[1:3]] if len(w) > 2 else [float(w[1]), 0.0])
                elif key == "vn":
                    vn.append([float(x) for x in w[1:4]])
                    if len(vn[-1]) != 3:
                        raise ValueError("vn takes 3 coordinates")
                elif key == "f":
                    if len(w) < 4:
                        raise ValueError("a face needs 3 corners")
                    cv, ct, cn = [], [], []
                    for tok in w[1:]:
                        parts = tok.split("/")
                        if len(parts) > 3:
                            raise ValueError(f"corner {tok!r}")
                        cv.append(index(parts[0], len(v), "v", ln))
                        ct.append(index(parts[1], len(vt), "vt", ln) if len(parts) > 1 and parts[1] else -1)
                        cn.append(index(parts[2], len(vn), "vn", ln) if len(parts) > 2 and parts[2] else -1)
                    for k in range(1, len(cv) - 1):
                        fv.append([cv[0], cv[k], cv[k + 1]])
                        ft.append([ct[0], ct[k], ct[k + 1]])
                        fn.append([cn[0], cn[k], cn[k + 1]])
                        fm.append(cur)
                elif key == "mtllib":
                    for name in w[1:]:
                        lib = os.path.join(base, name.replace("\\", "/"))
                        if not os.path.isfile(lib):
                            raise FileNotFoundError(f"{path}:{ln}: mtllib {name!r} not found at {lib}")
                        for k, m in read_mtl(lib).items():
                            materials[k] = m
                elif key == "usemtl":
                    name = " ".join(w[1:])
                    if name not in materials:
                        materials[name] = dict(Kd=None, Pr=None, map_Kd=None, map_Pr=None, norm=None)
                    cur = list(materials).index(name)
            except ValueError as e:
                if str(e).startswith(f"{path}:"):
                    raise
                raise ValueError(f"{path}:{ln}: unreadable line {line.strip()!r} ({e})") from None
    verts = np.asarray(v, np.float32).reshape(-1, 3)
    faces = np.asarray(fv, np.int32).reshape(-1, 3)
    fuv = np.asarray(ft, np.int32).reshape(-1, 3)
    fnn = np.asarray(fn, np.int32).reshape(-1, 3)
    uv = face_uv = None
    if len(vt) and faces.shape[0] and (fuv >= 0).all():
        uv, face_uv = np.asarray(vt, np.float32).reshape(-1, 2), fuv
    if len(vn) == len(v) and faces.shape[0] and np.array_equal(fnn, faces):
        normals = np.asarray(vn, np.float32).reshape(-1, 3)
    else:
        p = verts.astype(np.float64)
        g = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])  # length = twice the area
        acc = np.zeros_like(p)
        for k in range(3):
            np.add.at(acc, faces[:, k], g)
        n = np.linalg.norm(acc, axis=1, keepdims=True)
        normals = np.where(n > 0, acc / np.where(n > 0, n, 1.0), 0.0).astype(np.float32)
    return ObjMesh(verts, faces, uv, face_uv, normals, np.asarray(fm, np.int32), materials)
