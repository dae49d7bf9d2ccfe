"""Export of the learned geometry: field queries, sigma volumes, marching-tetrahedra meshes and PLY files.

Everything runs on the HIP device through the kernels of ``libpanonerf_hip.so`` (``pn_geometry.hip`` plus the MLP
entry points the renderer uses), under ``torch.no_grad()`` on the current stream.  CPU tensors raise: there is no host
fallback.  The only host synchronisation is the copy of the two mesh totals that sizes the outputs.

    query_field(model, points, ...)             sigma / albedo / rgb / normal / grad (d sigma / d mean) at [M, 3] points
    grid_points(bounds, resolution, ...)        the (mean, cov) rows of a grid's vertices
    density_grid(model, bounds, resolution)     sigma on an [nx, ny, nz] vertex grid
    marching_tetrahedra(sigma, level, bounds)   (vertices [V, 3], faces [F, 3] int32) of {sigma > level}
    extract_mesh(model, bounds, resolution, level)  Mesh(vertices, faces, normals, colors)
                                                (fusion.fused_mesh: the same Mesh from fused depth instead of a density level)
    write_ply(path, vertices, faces, normals, colors)  binary little-endian PLY
    read_ply(path)                              Mesh of host numpy arrays from such a file (binary or ASCII)
    read_obj(path)                              ObjMesh of host numpy arrays from a Wavefront OBJ (+ MTL) file
    triangle_atlas(faces, size)                 Atlas(uv, face_uv, size, cell): half a cell of a square image per face
    atlas_texels(vertices, faces, atlas)        per texel: face, bary, points, normals_g, normals_s, var
    atlas_rays(texels, offset)                  one short ray per owned texel, for bake_textures(method="ray")
    bake_textures(model, mesh, size, maps)      BakedMesh(vertices, faces, normals, uv, face_uv, maps): the field on a mesh
    write_obj(path, baked)                      OBJ + MTL + PNG / EXR images that read_obj and VirtualObject.from_obj read
    export_scene(model, bounds, resolution, level, path)   extract_mesh -> bake_textures -> write_obj

The mesh contract (edge ids, vertex and face order, winding) and the atlas layout are stated in include/panonerf_hip.h.
Out of scope of the baking: chart-based UV unwrapping, several materials, and mip levels above 0 (a per-triangle atlas
mixes neighbouring faces there: sample a baked asset at level 0, or let the engine re-atlas it).  Removing debris and
decimating a mesh before it is baked is ``meshops`` (export_scene's simplify / min_component_faces).
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
_CHUNK_RAYS = 1 << 15  # rays per renderer call of bake_textures(method="ray")


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


def _mesh_colors(model, colors):
    """the colour rule of extract_mesh and fusion.fused_mesh, with "auto" resolved for the model"""
    if colors not in ("auto", "albedo", "radiance", None):
        raise ValueError(f"colors must be 'auto', 'albedo', 'radiance' or None; got {colors!r}")
    if colors == "auto":
        colors = "albedo" if model._NC == 5 else "radiance"
    if colors == "albedo" and model._NC != 5:
        raise ValueError(f"colors='albedo' needs a PanoMipNeRF (5 density channels); {type(model).__name__} has none")
    return colors


def _field_mesh(model, verts, faces, variance, normals, colors, chunk_rows):
    """Mesh of (verts, faces) with the field queried at the vertices: the model's normals, and `colors` (_mesh_colors')"""
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


def extract_mesh(model, bounds, resolution, level, variance=None, normals=True, colors="auto", chunk_rows=None,
                 simplify=None, min_component_faces=None):
    """Mesh(vertices [V, 3], faces [F, 3] int32, normals [V, 3] | None, colors [V, 3] | None) of {sigma > level} on the
    model's device: density_grid -> marching_tetrahedra, then the field queried at the vertices with the grid's
    variance.  normals: the model's normals (-grad sigma, normalised).  colors: "auto" (albedo for PanoMipNeRF, radiance
    for MipNeRF), "albedo", "radiance" (rgb seen along -normal) or None.  min_component_faces / simplify (a cell size or a
    dict of simplify_mesh's keywords): meshops.clean_mesh between the extraction and the field query, so the normals and
    colours are the field's at the NEW vertices; with both None nothing of meshops runs."""
    colors = _mesh_colors(model, colors)
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
    if simplify is not None or min_component_faces is not None:
        from .meshops import clean_mesh
        verts, faces = clean_mesh(verts, faces, simplify, min_component_faces)
    return _field_mesh(model, verts, faces, variance, normals, colors, chunk_rows)


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


# ---------------------------------------------------------------------------------------- baking textures on a mesh
Atlas = collections.namedtuple("Atlas", ["uv", "face_uv", "size", "cell"])
BakedMesh = collections.namedtuple("BakedMesh", ["vertices", "faces", "normals", "uv", "face_uv", "maps"])

ATLAS_MIN_CELL = 6   # PN_ATLAS_MIN_CELL
ATLAS_MAX_SIZE = 16384  # PN_TEX_MAX_SIZE
BAKE_MAPS = ("albedo", "radiance", "normal", "normal_world", "coverage")


def atlas_cell(num_faces, size):
    """The cell size of the per-triangle atlas of `num_faces` faces in a size x size image: the largest c >= 6 with
    2 (size // c)^2 >= num_faces.  ValueError, naming the smallest size that would do, when there is none."""
    F, S = int(num_faces), int(size)
    if not 1 <= S <= ATLAS_MAX_SIZE:
        raise ValueError(f"the atlas size must be in [1, {ATLAS_MAX_SIZE}]; got {size!r}")
    if F < 0:
        raise ValueError(f"the number of faces must be >= 0; got {num_faces!r}")
    n = 1
    while 2 * n * n < F:  # cells per row needed: the smallest n with 2 n^2 >= F
        n += 1
    c = S // n  # the largest c with S // c >= n
    if c < ATLAS_MIN_CELL:
        need = ATLAS_MIN_CELL * n
        hint = f"size >= {need} would do" if need <= ATLAS_MAX_SIZE else \
            f"that takes size {need}, above the largest texture ({ATLAS_MAX_SIZE}): bake a coarser mesh"
        raise ValueError(f"an atlas of {S} x {S} texels is too small for {F} faces ({n} x {n} cells of at least "
                         f"{ATLAS_MIN_CELL} texels): {hint}")
    return c


def _atlas_args(faces, size, cell):
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be an [F, 3] tensor; got {getattr(faces, 'shape', type(faces))}")
    F, S = int(faces.shape[0]), int(size)
    c = atlas_cell(F, S)
    if cell is not None:
        if not ATLAS_MIN_CELL <= int(cell) <= c:
            raise ValueError(f"cell must be in [{ATLAS_MIN_CELL}, {c}] for {F} faces in {S} x {S} texels; got {cell!r}")
        c = int(cell)
    return F, S, c


def triangle_atlas(faces, size, cell=None):
    """Atlas(uv [3F, 2] fp32, face_uv [F, 3] int32, size, cell) of the per-triangle atlas (include/panonerf_hip.h, "baking"):
    every face gets half a cell of cell x cell texels of a size x size image, with a one-texel gutter that carries the
    continuation of the face's own plane, so that a level-0 bilinear sample anywhere on the face reads its own texels only.
    cell: None picks the largest that fits (atlas_cell).  Works on any triangle soup; needs no connectivity."""
    dev = _device_of(faces)
    F, S, c = _atlas_args(faces, size, cell)
    with torch.no_grad(), torch.cuda.device(dev):
        uv = torch.empty(3 * F, 2, dtype=torch.float32, device=dev)
        _lib.call("pn_atlas_uv", F, S, c, _lib.ptr(uv) if F else None, _lib.stream(dev))
        face_uv = torch.arange(3 * F, dtype=torch.int32, device=dev).view(F, 3)
    return Atlas(uv, face_uv, S, c)


def _mesh_tensors(vertices, faces, normals):
    dev = _device_of(vertices, faces, *([normals] if normals is not None else []))
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"vertices must be [V, 3] and faces [F, 3]; got {tuple(vertices.shape)}, {tuple(faces.shape)}")
    v = vertices.detach().to(torch.float32).contiguous()
    f = faces.detach().to(torch.int32).contiguous()
    n = None
    if normals is not None:
        if tuple(normals.shape) != tuple(v.shape):
            raise ValueError(f"normals must be [V, 3] like the vertices; got {tuple(normals.shape)}")
        n = normals.detach().to(torch.float32).contiguous()
    return dev, v, f, n


def atlas_texels(vertices, faces, atlas, normals=None):
    """What every texel of the atlas shows, as a dict of [S, S, ...] device tensors: face (int32, -1: unowned), bary [.., 2]
    (the texel centre in its face, extrapolated in the gutter), points [.., 3], normals_g (geometric), normals_s (the
    blend of the vertex `normals`, not flipped; normals_g without them) and var (the per-axis second moment of the
    texel's square footprint on the face, for the integrated encoding)."""
    dev, v, f, n = _mesh_tensors(vertices, faces, normals)
    S, c = int(atlas.size), int(atlas.cell)
    e = lambda *s: torch.empty(S, S, *s, dtype=torch.float32, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        out = dict(face=torch.empty(S, S, dtype=torch.int32, device=dev), bary=e(2), points=e(3), normals_g=e(3),
                   normals_s=e(3), var=e())
        _lib.call("pn_atlas_texels", S, c, int(f.shape[0]), int(v.shape[0]), _lib.ptr(v), _lib.ptr(f), _lib.ptr(n),
                  out["face"].data_ptr(), out["bary"].data_ptr(), out["points"].data_ptr(), out["normals_g"].data_ptr(),
                  out["normals_s"].data_ptr(), out["var"].data_ptr(), _lib.stream(dev))
    return out


def _median_texel_side(var):
    """the side of the median owned texel's footprint: var = side^2 / 12"""
    return float(torch.sqrt(12.0 * var.median())) if var.numel() else 0.0


def atlas_rays(texels, offset=None):
    """(Rays of the M owned texels, their flat indices [M] into the S x S image): one short ray per texel, from
    points + offset normals_g along -normals_g, near = 0, far = 2 offset, radii = sqrt(12 var) / (2 offset) - a cone one
    texel wide where it meets the face.  offset: None is four sides of the median texel (read back from the device).
    Synchronises for the count of owned texels."""
    face = texels["face"]
    dev = _device_of(face)
    with torch.no_grad(), torch.cuda.device(dev):
        idx = torch.nonzero(face.reshape(-1) >= 0).reshape(-1)
        return _atlas_rays(texels, idx, offset, dev), idx


def _atlas_rays(texels, idx, offset, dev):
    from .rays import Rays
    var = texels["var"].reshape(-1)[idx]
    if offset is None:
        offset = 4.0 * _median_texel_side(var)
    offset = float(offset)
    if not offset > 0.0:
        raise ValueError(f"offset must be positive; got {offset!r} (a mesh of zero-area faces has no default)")
    ng = texels["normals_g"].reshape(-1, 3)[idx]
    o = texels["points"].reshape(-1, 3)[idx] + offset * ng
    d = -ng
    col = lambda x: torch.full((idx.shape[0], 1), float(x), dtype=torch.float32, device=dev)
    radii = (torch.sqrt(12.0 * var) / (2.0 * offset)).reshape(-1, 1)
    return Rays(o, d, d.clone(), radii, col(1.0), col(0.0), col(2.0 * offset), col(0.0))


def _bake_values(source, want, method, idx, pts, var, ns, tex, offset, chunk_rows, env_rays):
    """name -> [M, 3] for the names in `want` ("albedo", "radiance", "normal") at the owned texels"""
    if callable(source) and not isinstance(source, torch.nn.Module):
        got = source(pts, var, ns)
        missing = [k for k in want if k not in got]
        if missing:
            raise ValueError(f"the field callable returned {sorted(got)}; the maps asked for need {missing} too")
        for k in want:
            if tuple(got[k].shape) != tuple(pts.shape):
                raise ValueError(f"the field callable's {k!r} must be [M, 3] like the points; got {tuple(got[k].shape)}")
        return {k: got[k].to(torch.float32) for k in want}
    model = source
    if "albedo" in want and model._NC != 5:
        raise ValueError(f"albedo needs a 5-channel density head (PanoMipNeRF); {type(model).__name__} has {model._NC}")
    if method == "point":
        var3 = var[:, None].expand(-1, 3).contiguous()
        outs = tuple(k for k in ("albedo", "normal") if k in want)
        res = query_field(model, pts, var3, outputs=outs, chunk_rows=chunk_rows) if outs else {}
        if "radiance" in want:
            res["radiance"] = query_field(model, pts, var3, viewdirs=-ns, outputs=("rgb",), chunk_rows=chunk_rows)["rgb"]
        return res
    # method == "ray": one short ray per owned texel through the renderer; the fine level's rgb, normal and albedo
    rays = _atlas_rays(tex, idx, offset, pts.device)
    M = int(pts.shape[0])
    chunk = int(chunk_rows) if chunk_rows else _CHUNK_RAYS
    if chunk <= 0:
        raise ValueError(f"chunk_rows must be positive; got {chunk_rows!r}")
    surf = "albedo" in want
    if surf and env_rays is None:
        raise ValueError("method='ray' composites the albedo in the renderer's surface pass, which needs env_rays "
                         "(rays.generate_lit_rays); pass env_rays=, or bake the albedo with method='point'")
    parts = {k: [] for k in want}
    for first in range(0, M, chunk):
        sub = type(rays)(*[x[first:first + chunk] for x in rays])
        if model._NC == 5:
            _, fine = model(rays=sub, env_rays=env_rays if surf else None, randomized=False, white_bkgd=False,
                            enable_surf=surf, use_ort_loss=False)
        else:  # a MipNeRF composites its normals only with the orientation term on
            _, fine = model(rays=sub, randomized=False, white_bkgd=False, use_ort_loss=True)
        for k, v in (("radiance", fine[0]), ("normal", fine[3]), ("albedo", fine[4] if surf else None)):
            if k in want:
                parts[k].append(v)
    return {k: (torch.cat(v) if len(v) > 1 else v[0]) for k, v in parts.items()}


def bake_textures(model, mesh, size=1024, maps=("albedo", "normal"), method="point", offset=None, cell=None,
                  chunk_rows=None, env_rays=None):
    """Bake the field onto `mesh` (anything with vertices, faces and normals | None, e.g. extract_mesh's Mesh):
    BakedMesh(vertices, faces, normals, uv, face_uv, maps) with maps a dict of [S, S, 3] fp32 device images over the
    per-triangle atlas of triangle_atlas(faces, size, cell).

    maps: "albedo" (PanoMipNeRF only), "radiance" (the HDR rgb seen along -normals_s), "normal" (the field's normal in the
    tangent space objects.VirtualObject decodes; (0.5, 0.5, 1) where it faces away from the mesh's own normal),
    "normal_world" (the same before encoding) and "coverage" ([S, S, 1]: 1 on owned texels).  Unowned texels are 0.
    method="point" is query_field at the owned texels' points with their footprint variance - bit for bit.
    method="ray" renders one short ray per owned texel (atlas_rays: from `offset` above the face to `offset` below it, a
    cone one texel wide at the face; offset None = four sides of the median texel) and takes the fine level's rgb, normal
    and albedo (the radiance is then seen along the ray, -normals_g) - bit for bit the model called on atlas_rays(...).  It
    is the mode for a coarse mesh that sits off the true level set.  The renderer composites the albedo in its surface
    pass, so "albedo" then needs env_rays (as the model's forward does); chunk_rows counts rays per call here.
    `model` may be a callable f(points [M, 3], var [M], normals [M, 3]) -> dict of [M, 3] tensors under the names
    "albedo", "radiance", "normal" instead.  Mip levels above 0 of a per-triangle atlas mix neighbouring faces: sample the
    result at level 0 (hit_attributes(radii=None)).  One host synchronisation: the count of owned texels (and, for
    method="ray" without an offset, the median texel's side)."""
    maps = tuple(maps)
    bad = [m for m in maps if m not in BAKE_MAPS]
    if bad or not maps:
        raise ValueError(f"unknown maps {bad}; choose from {BAKE_MAPS}")
    is_model = isinstance(model, torch.nn.Module)
    if not is_model and not callable(model):
        raise ValueError(f"model must be a MipNeRF / PanoMipNeRF or a callable; got {type(model).__name__}")
    if is_model and "albedo" in maps and model._NC != 5:
        raise ValueError(f"albedo needs a 5-channel density head (PanoMipNeRF); {type(model).__name__} has {model._NC}")
    if method not in ("point", "ray"):
        raise ValueError(f"method must be 'point' or 'ray'; got {method!r}")
    dev, v, f, n = _mesh_tensors(mesh.vertices, mesh.faces, getattr(mesh, "normals", None))
    if is_model and _model_device(model) != dev:
        raise RuntimeError(f"the mesh is on {dev}, the model on {_model_device(model)}")
    atlas = triangle_atlas(f, size, cell)
    tex = atlas_texels(v, f, atlas, n)
    S = atlas.size
    want = tuple(k for k, users in (("albedo", ("albedo",)), ("radiance", ("radiance",)), ("normal", ("normal", "normal_world")))
                 if any(u in maps for u in users))
    with torch.no_grad(), torch.cuda.device(dev):
        idx = torch.nonzero(tex["face"].reshape(-1) >= 0).reshape(-1)  # the one host sync
        out = {}
        vals = {}
        if want and idx.numel():
            vals = _bake_values(model, want, method, idx, tex["points"].reshape(-1, 3)[idx], tex["var"].reshape(-1)[idx],
                                tex["normals_s"].reshape(-1, 3)[idx], tex, offset, chunk_rows, env_rays)
        images = {}
        for k in want:
            img = torch.zeros(S * S, 3, dtype=torch.float32, device=dev)
            if k in vals:
                img[idx] = vals[k]
            images[k] = img.view(S, S, 3)
        for m in maps:
            if m in ("albedo", "radiance"):
                out[m] = images[m]
            elif m == "normal_world":
                out[m] = images["normal"]
            elif m == "normal":
                enc = torch.empty(S, S, 3, dtype=torch.float32, device=dev)
                _lib.call("pn_atlas_encode_normals", S, atlas.cell, int(f.shape[0]), int(v.shape[0]), _lib.ptr(v),
                          _lib.ptr(f), _lib.ptr(atlas.uv), tex["face"].data_ptr(), tex["normals_s"].data_ptr(),
                          images["normal"].data_ptr(), enc.data_ptr(), _lib.stream(dev))
                out[m] = enc
            else:
                out[m] = (tex["face"] >= 0).to(torch.float32).view(S, S, 1)
    return BakedMesh(v, f, n, atlas.uv, atlas.face_uv, out)


def quantize_image(image, srgb=False, table=True):
    """fp32 device image [..., C] (C <= 4) -> uint8 of the same shape through pn_atlas_quantize: the code whose decoded
    value (objects.Texture's table: the sRGB EOTF, or i / 255) is nearest, so that Texture(bytes, srgb=srgb) inverts it as
    well as 8 bits allow; table=False is round-half-even(255 clamp(x))."""
    from .objects import _decode_table
    dev = _device_of(image)
    x = image.detach().to(torch.float32).contiguous()
    C = int(x.shape[-1]) if x.dim() else 0
    if not 1 <= C <= 4:
        raise ValueError(f"image must be [..., C] with 1 <= C <= 4; got {tuple(image.shape)}")
    with torch.no_grad(), torch.cuda.device(dev):
        out = torch.empty(x.shape, dtype=torch.uint8, device=dev)
        tab = torch.from_numpy(_decode_table(srgb)).to(dev) if table else None
        _lib.call("pn_atlas_quantize", x.numel() // C, C, _lib.ptr(x) if x.numel() else None, _lib.ptr(tab),
                  _lib.ptr(out) if x.numel() else None, _lib.stream(dev))
        if tab is not None:
            tab.record_stream(torch.cuda.current_stream(dev))
    return out


def _image_bytes(img, srgb):
    """a map as uint8 host bytes: uint8 is taken as it is, fp32 goes through the device quantiser"""
    if isinstance(img, torch.Tensor):
        if img.dtype == torch.uint8:
            return img.detach().cpu().numpy()
        return quantize_image(img, srgb=srgb).cpu().numpy()
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise RuntimeError("a floating map on the host cannot be written as PNG: the quantiser runs on the HIP device "
                           "(there is no CPU fallback); pass a device tensor, uint8 bytes, or image_format='exr'")
    return a


def _image_f32(img):
    a = img.detach().cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    if a.dtype == np.uint8:
        raise ValueError("a uint8 map cannot be written as EXR; pass image_format='png'")
    return np.ascontiguousarray(a, dtype=np.float32)


def write_obj(path, baked, image_format="png", srgb=True):
    """Write a BakedMesh as Wavefront OBJ + MTL + images, and return {map name: image path}: `path` (v, vn when there are
    normals, vt, f v/vt[/vn], mtllib, usemtl; floats as %.9g, which round-trips fp32), <stem>.mtl (map_Kd for "albedo",
    norm for "normal", map_Ke for "radiance") and <stem>_albedo / <stem>_normal as .png (8 bits through pn_atlas_quantize:
    the albedo against the sRGB table when `srgb`, the normal map linear) or .exr (fp32) by image_format; "radiance" is HDR
    and always goes to <stem>_radiance.exr.  "normal_world" and "coverage" are not written.  read_obj and
    objects.VirtualObject.from_obj read the result with their defaults."""
    from . import io_exr
    if image_format not in ("png", "exr"):
        raise ValueError(f"image_format must be 'png' or 'exr'; got {image_format!r}")
    v = _host(baked.vertices, np.float32, "vertices")
    f = _host(baked.faces, np.int32, "faces")
    n = None if baked.normals is None else _host(baked.normals, np.float32, "normals")
    uv = baked.uv.detach().cpu().numpy() if isinstance(baked.uv, torch.Tensor) else np.asarray(baked.uv)
    uv = np.ascontiguousarray(uv, dtype=np.float32)
    fuv = _host(baked.face_uv, np.int32, "face_uv")
    if uv.ndim != 2 or uv.shape[1] != 2 or fuv.shape != f.shape:
        raise ValueError(f"uv must be [T, 2] and face_uv [F, 3] like the faces; got {uv.shape}, {fuv.shape}")
    if n is not None and n.shape != v.shape:
        raise ValueError(f"normals must be [V, 3] like the vertices; got {n.shape}")
    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    written = {}
    for key, statement in (("albedo", "map_Kd"), ("normal", "norm"), ("radiance", "map_Ke")):
        img = baked.maps.get(key)
        if img is None:
            continue
        ext = "exr" if key == "radiance" else image_format
        file = f"{stem}_{key}.{ext}"
        if ext == "exr":
            io_exr.write_exr(file, _image_f32(img))
        else:
            io_exr.write_png(file, _image_bytes(img, srgb and key == "albedo"))
        written[key] = (statement, file)
    with open(stem + ".mtl", "w") as fh:
        fh.write(f"newmtl {name}\nKd 1 1 1\n")
        for key, (statement, file) in written.items():
            fh.write(f"{statement} {os.path.basename(file)}\n")
    g = lambda row: " ".join("%.9g" % x for x in row)
    lines = [f"mtllib {name}.mtl"]
    lines += ["v " + g(r) for r in v]
    if n is not None:
        lines += ["vn " + g(r) for r in n]
    lines += ["vt " + g(r) for r in uv]
    lines.append(f"usemtl {name}")
    if n is not None:
        lines += ["f " + " ".join(f"{a + 1}/{t + 1}/{a + 1}" for a, t in zip(fa, ft)) for fa, ft in zip(f, fuv)]
    else:
        lines += ["f " + " ".join(f"{a + 1}/{t + 1}" for a, t in zip(fa, ft)) for fa, ft in zip(f, fuv)]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return {k: file for k, (_, file) in written.items()}


def export_scene(model, bounds, resolution, level, path, size=1024, image_format="png", srgb=True, simplify=None,
                 min_component_faces=None, **bake_kw):
    """extract_mesh -> bake_textures -> write_obj: the scene as a textured mesh at `path`; returns the BakedMesh.
    bake_kw goes to bake_textures (maps, method, offset, cell, chunk_rows, env_rays).  min_component_faces drops the
    components with fewer faces and simplify (a cell size, or a dict of meshops.simplify_mesh's keywords such as
    {"target_faces": 20000}) decimates the mesh before it is baked: the normal map then carries the detail the
    decimation removed.  With both None the result is what it was without them, bit for bit."""
    mesh = extract_mesh(model, bounds, resolution, level, colors=None, chunk_rows=bake_kw.get("chunk_rows"),
                        simplify=simplify, min_component_faces=min_component_faces)
    baked = bake_textures(model, mesh, size=size, **bake_kw)
    write_obj(path, baked, image_format=image_format, srgb=srgb)
    return baked
