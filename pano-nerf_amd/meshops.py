"""Cleaning and simplifying exported meshes: connected components, debris removal and quadric vertex clustering.

``geometry.extract_mesh`` and ``fusion.fused_mesh`` hand over what marching tetrahedra leaves behind: a face count that
follows the grid instead of the surface, and every scrap of density above the level as an island of its own.  This module
holds the two standard steps of a mesh export that come between extraction and baking:

    mesh_components(faces, num_vertices)        (vertex_label [V], face_label [F] int32, count): faces that share a vertex index
    component_stats(vertices, faces, face_label, count)   per component: faces, vertices, area, signed volume, bounding box
    filter_components(mesh, min_faces, min_area, keep_largest, by)   (Mesh, vertex_map, face_map) without the floaters
    simplify_mesh(mesh, cell | target_faces, origin, lam)  (Mesh, vertex_map, face_map, flags): quadric vertex clustering
    edge_counts(faces)                          {"boundary", "nonmanifold", "inconsistent"}: what that did to the topology
    clean_mesh(vertices, faces, simplify, min_component_faces)   the two steps as export_scene and fused_mesh run them

Everything that computes is a HIP kernel of ``pn_meshops.hip`` (union-find with 32-bit atomicMin, fp64 sums over the fp32
inputs in an order fixed by the input alone, the 3 x 3 solve); torch does the sorts, scans, ``unique_consecutive`` and
gathers in between, as it does for the BVH and the emitters.  Everything runs on the HIP device under ``torch.no_grad()`` on
the current stream; CPU tensors raise, there is no host fallback.  The host synchronisations are the copies of the totals
that size the outputs (the component count, the cluster count, the surviving faces) and the two validation flags.  The
contract - cells, quadric, solve, the order of every sum - is stated in include/panonerf_hip.h, section "mesh operations",
and discussed in DESIGN.md 6l; two calls on the same input give the same bits.

Out of scope: topology preservation (clustering can pinch a thin wall into non-manifold edges: edge_counts says so),
boundary-edge quadrics for open meshes, edge-collapse QEM, smoothing, and UV-preserving decimation (bake after
simplifying: the normal map then carries what was removed).
"""
import math

import numpy as np
import torch

from . import _lib
from .geometry import Mesh, _device_of

_BY = ("area", "faces", "vertices", "volume")
STATS_CHUNK = 4096  # faces per workgroup of the component records (kChunk of pn_meshops.hip)
MAX_CLUSTERS = 1 << 21  # three cluster ranks share one 63-bit face key


def _as_mesh(mesh, faces=None):
    """Mesh of a Mesh-like object or of (vertices, faces); tensors are checked, not converted"""
    if faces is not None:
        mesh = Mesh(mesh, faces, None, None)
    elif isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        mesh = Mesh(mesh[0], mesh[1], None, None)
    v, f = mesh.vertices, mesh.faces
    n, c = getattr(mesh, "normals", None), getattr(mesh, "colors", None)
    for name, t, dt in (("vertices", v, torch.float32), ("faces", f, torch.int32), ("normals", n, torch.float32),
                        ("colors", c, torch.float32)):
        if t is None and name in ("normals", "colors"):
            continue
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name} must be an [N, 3] tensor; got {getattr(t, 'shape', type(t))}")
        if t.dtype != dt:
            raise ValueError(f"{name} must be {dt}; got {t.dtype}")
    dev = _device_of(*[t for t in (v, f, n, c) if t is not None])
    for name, t in (("faces", f), ("normals", n), ("colors", c)):
        if t is not None and t.device != dev:
            raise RuntimeError(f"the {name} are on {t.device} but the vertices on {dev}")
    for name, t in (("normals", n), ("colors", c)):
        if t is not None and t.shape[0] != v.shape[0]:
            raise ValueError(f"{name} must be [V, 3] like the vertices; got {tuple(t.shape)}")
    if v.shape[0] >= 1 << 31 or f.shape[0] >= 1 << 31:
        raise ValueError("a mesh of 2^31 or more vertices or faces does not fit int32 indices")
    g = lambda t: None if t is None else t.detach().contiguous()
    return Mesh(g(v), g(f), g(n), g(c)), dev


def _check(v, f, V, dev):
    """the two rules every function shares: finite vertices (v may be None: not looked at), face indices in [0, V)"""
    F = int(f.shape[0])
    if V == 0 and F == 0:
        return
    bad = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.call("pn_mesh_check", V, F, _lib.ptr(v) if V else None, _lib.ptr(f) if F else None, bad.data_ptr(), _lib.stream(dev))
    nonfinite, outside = (int(x) for x in bad.cpu())  # one copy of the two flags
    if nonfinite:
        raise ValueError("the vertices hold a NaN or an infinity")
    if outside:
        raise ValueError(f"a face index lies outside [0, {V})")


def _faces_arg(faces, num_vertices):
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be an [F, 3] tensor; got {getattr(faces, 'shape', type(faces))}")
    if faces.dtype != torch.int32:
        raise ValueError(f"faces must be int32; got {faces.dtype}")
    V = int(num_vertices)
    if V != num_vertices or V < 0 or V >= 1 << 31 or faces.shape[0] >= 1 << 31:
        raise ValueError(f"num_vertices must be an integer in [0, 2^31); got {num_vertices!r}")
    return faces.detach().contiguous(), V, _device_of(faces)


# ------------------------------------------------------------------------------------------------------- components
def _components(f, V, dev):
    F = int(f.shape[0])
    vlab = torch.empty(V, dtype=torch.int32, device=dev)
    flab = torch.empty(F, dtype=torch.int32, device=dev)
    if V == 0:
        return vlab, flab, 0
    st = _lib.stream(dev)
    parent = torch.empty(V, dtype=torch.int32, device=dev)
    roots = torch.empty(V, dtype=torch.int32, device=dev)
    flags = torch.empty(V, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("pn_mesh_components", V, F, _lib.ptr(f) if F else None, parent.data_ptr(), roots.data_ptr(), flags.data_ptr(), st)
    prefix = torch.cumsum(flags, 0, dtype=torch.int32)  # roots are numbered by a prefix count, as the emitters' are
    _lib.call("pn_mesh_labels", V, F, _lib.ptr(f) if F else None, roots.data_ptr(), prefix.data_ptr(), vlab.data_ptr(),
              _lib.ptr(flab) if F else None, count.data_ptr(), st)
    return vlab, flab, int(count)  # the host sync: sizes the records


def mesh_components(faces, num_vertices):
    """(vertex_label int32 [V], face_label int32 [F], count): the connected components of a mesh, two faces being connected
    when they share a vertex INDEX (vertices at the same position under different indices do not connect).  Components are
    numbered 0 .. count - 1 in ascending order of their smallest vertex index; a vertex no face uses gets -1 and forms no
    component.  count is a host int (the one synchronisation).  Union-find over the vertices with 32-bit atomicMin: the
    labels do not depend on the schedule, and repeated calls give the same bits."""
    f, V, dev = _faces_arg(faces, num_vertices)
    with torch.no_grad(), torch.cuda.device(dev):
        _check(None, f, V, dev)
        return _components(f, V, dev)


def _stats(v, f, flab, vlab, C, dev):
    z = lambda *s, dt=torch.float32: torch.zeros(C, *s, dtype=dt, device=dev)
    out = dict(faces=z(dt=torch.int32), vertices=z(dt=torch.int32), area=z(), volume=z(), bbox=z(6))
    if C == 0:
        return out
    F, V = int(f.shape[0]), int(v.shape[0])
    key = torch.where((flab >= 0) & (flab < C), flab, C).to(torch.int64)
    skey, order = torch.sort(key, stable=True)  # face order kept within a component
    starts = torch.searchsorted(skey, torch.arange(C + 1, dtype=torch.int64, device=dev))
    nch = (starts[1:] - starts[:-1] + (STATS_CHUNK - 1)) // STATS_CHUNK  # chunks of 4096 faces, one workgroup each
    cstarts = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    cstarts[1:] = torch.cumsum(nch, 0)
    B = F // STATS_CHUNK + C  # bounds the number of chunks without a host copy
    work = torch.empty(max(B, 1), 10, dtype=torch.float64, device=dev)
    _lib.call("pn_mesh_component_stats", V, F, C, v.data_ptr(), f.data_ptr(), order.data_ptr(), starts.data_ptr(),
              cstarts.data_ptr(), B, work.data_ptr(), vlab.data_ptr(), out["faces"].data_ptr(), out["vertices"].data_ptr(),
              out["area"].data_ptr(), out["volume"].data_ptr(), out["bbox"].data_ptr(), _lib.stream(dev))
    return out


def _vertex_labels(f, flab, V, dev):
    """vertex labels from face labels: every corner of a face carries the face's label (-1 for an unused vertex)"""
    vlab = torch.full((V,), -1, dtype=torch.int32, device=dev)
    if f.shape[0]:
        vlab[f.reshape(-1).to(torch.int64)] = flab.repeat_interleave(3)
    return vlab


def component_stats(vertices, faces, face_label, count):
    """The record of every component, a dict of [count, ...] device tensors: "faces" and "vertices" (int32 counts), "area"
    (sum |n| / 2), "volume" (the signed volume sum a . (b x c) / 6: positive for a closed component wound outwards, and
    meaningless for an open one) and "bbox" [count, 6] (min then max).  The faces are grouped by label with one stable
    torch.sort and summed in chunks of 4096 in fp64 in a fixed order (include/panonerf_hip.h), so the cost
    follows the faces plus the components, not their product, and the bits repeat."""
    mesh, dev = _as_mesh(vertices, faces)
    v, f = mesh.vertices, mesh.faces
    C = int(count)
    if C != count or C < 0 or C > v.shape[0]:
        raise ValueError(f"count must be an integer in [0, V]; got {count!r}")
    if not isinstance(face_label, torch.Tensor) or face_label.dtype != torch.int32 or tuple(face_label.shape) != (f.shape[0],):
        raise ValueError(f"face_label must be an int32 [{f.shape[0]}] tensor; got {getattr(face_label, 'dtype', type(face_label))} "
                         f"{getattr(face_label, 'shape', '')}")
    _device_of(face_label)
    with torch.no_grad(), torch.cuda.device(dev):
        _check(v, f, int(v.shape[0]), dev)
        flab = face_label.detach().contiguous()
        return _stats(v, f, flab, _vertex_labels(f, flab, int(v.shape[0]), dev), C, dev)


def _compact(mesh, keep_face, dev):
    """the faces with keep_face and the vertices they use, both in their original relative order"""
    v, f = mesh.vertices, mesh.faces
    V = int(v.shape[0])
    face_map = torch.nonzero(keep_face).reshape(-1)  # host sync: sizes the outputs
    kept = f[face_map]
    used = torch.zeros(V, dtype=torch.bool, device=dev)
    used[kept.reshape(-1).to(torch.int64)] = True
    new = torch.cumsum(used, 0, dtype=torch.int32) - 1
    vertex_map = torch.where(used, new, torch.full_like(new, -1))
    sel = torch.nonzero(used).reshape(-1)
    g = lambda t: None if t is None else t[sel]
    out = Mesh(v[sel], vertex_map[kept.to(torch.int64)].to(torch.int32), g(mesh.normals), g(mesh.colors))
    return out, vertex_map, face_map.to(torch.int32)


def filter_components(mesh, min_faces=0, min_area=0.0, keep_largest=None, by="area"):
    """(Mesh, vertex_map int32 [V], face_map int32 [F']): the mesh with only the components that have at least min_faces
    faces and at least min_area area and, with keep_largest = n, only the n largest of those by `by` ("area", "faces",
    "vertices" or "volume" = |signed volume|; ties go to the lower label).  Vertices (with their normals and colours) and
    faces keep their original relative order; vertex_map takes an old vertex index to its new one (-1: dropped), face_map a
    new face index to its old one.  Vertices no face uses are dropped.  mesh: a Mesh or (vertices, faces)."""
    mesh, dev = _as_mesh(mesh)
    if by not in _BY:
        raise ValueError(f"by must be one of {_BY}; got {by!r}")
    mf, ma = int(min_faces), float(min_area)
    if mf != min_faces or mf < 0 or not ma >= 0.0:
        raise ValueError(f"min_faces must be a non-negative integer and min_area >= 0; got {min_faces!r}, {min_area!r}")
    if keep_largest is not None and (int(keep_largest) != keep_largest or keep_largest < 0):
        raise ValueError(f"keep_largest must be None or a non-negative integer; got {keep_largest!r}")
    v, f = mesh.vertices, mesh.faces
    V, F = int(v.shape[0]), int(f.shape[0])
    with torch.no_grad(), torch.cuda.device(dev):
        _check(v, f, V, dev)
        if F == 0:
            return (Mesh(v[:0], f, None if mesh.normals is None else mesh.normals[:0],
                         None if mesh.colors is None else mesh.colors[:0]),
                    torch.full((V,), -1, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev))
        vlab, flab, C = _components(f, V, dev)
        st = _stats(v, f, flab, vlab, C, dev)
        keep = (st["faces"] >= mf) & (st["area"] >= ma)
        if keep_largest is not None:
            size = {"area": st["area"], "faces": st["faces"].to(torch.float32), "vertices": st["vertices"].to(torch.float32),
                    "volume": st["volume"].abs()}[by]
            size = torch.where(keep, size, torch.full_like(size, -1.0))  # the dropped ones sort last
            order = torch.sort(size, descending=True, stable=True)[1]  # stable: ties go to the lower label
            top = torch.zeros(C, dtype=torch.bool, device=dev)
            top[order[:int(keep_largest)]] = True
            keep &= top
        return _compact(mesh, keep[flab.to(torch.int64)], dev)


# --------------------------------------------------------------------------------------------------- simplification
def _cells(v, cell, origin):
    """(lo (3 floats as fp32 values), cell as an fp32 value, n (3 ints)) of the cell grid over the vertices: two host copies
    (the minimum and the maximum), which size the key space"""
    c = float(np.float32(cell))
    if not (c > 0.0 and math.isfinite(c)):
        raise ValueError(f"cell must be positive and finite in fp32; got {cell!r}")
    vmin, vmax = (t.cpu().numpy() for t in (v.amin(0), v.amax(0)))
    if origin is None:
        lo = vmin
    else:
        lo = np.asarray(origin, dtype=np.float64).reshape(-1).astype(np.float32)
        if lo.shape != (3,) or not np.isfinite(lo).all():
            raise ValueError(f"origin must be 3 finite numbers; got {origin!r}")
    n = []
    for a in range(3):
        q = math.floor((float(vmax[a]) - float(lo[a])) / c)  # the kernel's own fp64 expression, at the largest vertex
        n.append(int(max(q, 0)) + 1)
    if n[0] * n[1] * n[2] >= 1 << 63:
        raise ValueError(f"a cell of {c} gives {n[0]} x {n[1]} x {n[2]} cells, whose key does not fit 63 bits: use a larger cell")
    return tuple(float(x) for x in lo), c, tuple(n)


def _cluster(v, f, lo, cell, n, dev):
    """keys -> clusters -> remapped faces and the survivors; no solve.  Returns a dict of device tensors and K."""
    V, F = int(v.shape[0]), int(f.shape[0])
    st = _lib.stream(dev)
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    _lib.call("pn_cluster_keys", V, v.data_ptr(), *lo, cell, *n, keys.data_ptr(), st)
    skey, vorder = torch.sort(keys, stable=True)  # vertex order kept within a cluster
    ckeys, inverse, counts = torch.unique_consecutive(skey, return_inverse=True, return_counts=True)
    K = int(ckeys.shape[0])  # host sync: sizes the clusters
    if K >= MAX_CLUSTERS:
        raise ValueError(f"a cell of {cell} gives {K} clusters; the face keys hold at most 2^21 - 1: use a larger cell")
    rank = torch.empty(V, dtype=torch.int32, device=dev)
    rank[vorder] = inverse.to(torch.int32)
    vstarts = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    vstarts[1:] = torch.cumsum(counts, 0)
    rf = torch.empty(F, 3, dtype=torch.int32, device=dev)
    fkey = torch.empty(F, dtype=torch.int64, device=dev)
    _lib.call("pn_cluster_faces", F, V, K, _lib.ptr(f) if F else None, rank.data_ptr(), _lib.ptr(rf) if F else None,
              _lib.ptr(fkey) if F else None, st)
    sk, forder = torch.sort(fkey, stable=True)  # the lowest face index comes first within a key
    first = torch.ones(F, dtype=torch.bool, device=dev)
    first[1:] = sk[1:] != sk[:-1]
    first &= sk != torch.iinfo(torch.int64).max
    keep = torch.zeros(F, dtype=torch.bool, device=dev)
    keep[forder] = first
    return dict(keys=keys, ckeys=ckeys, rank=rank, vorder=vorder, vstarts=vstarts, faces=rf, keep=keep), K


def _count_faces(v, f, lo, cell, n, dev):
    c, _ = _cluster(v, f, lo, cell, n, dev)
    return int(c["keep"].sum())


def _simplify(mesh, lo, cell, n, lam, dev):
    v, f = mesh.vertices, mesh.faces
    V, F = int(v.shape[0]), int(f.shape[0])
    c, K = _cluster(v, f, lo, cell, n, dev)
    st = _lib.stream(dev)
    # the (face, corner) incidences grouped by the cluster of the corner's vertex, ascending 3 f + corner within one
    inc = c["rank"][f.reshape(-1).to(torch.int64)].to(torch.int64)
    sinc, iorder = torch.sort(inc, stable=True)
    istarts = torch.searchsorted(sinc, torch.arange(K + 1, dtype=torch.int64, device=dev))
    pos = torch.empty(K, 3, dtype=torch.float32, device=dev)
    nrm = None if mesh.normals is None else torch.empty(K, 3, dtype=torch.float32, device=dev)
    col = None if mesh.colors is None else torch.empty(K, 3, dtype=torch.float32, device=dev)
    flags = torch.empty(K, dtype=torch.uint8, device=dev)
    _lib.call("pn_cluster_solve", K, V, F, v.data_ptr(), _lib.ptr(f) if F else None, _lib.ptr(mesh.normals), _lib.ptr(mesh.colors),
              *lo, cell, *n, c["ckeys"].data_ptr(), c["vorder"].data_ptr(), c["vstarts"].data_ptr(),
              _lib.ptr(iorder) if F else None, istarts.data_ptr(), lam, pos.data_ptr(), _lib.ptr(nrm), _lib.ptr(col),
              flags.data_ptr(), st)
    face_map = torch.nonzero(c["keep"]).reshape(-1)  # host sync: sizes the outputs
    kept = c["faces"][face_map].to(torch.int64)
    used = torch.zeros(K, dtype=torch.bool, device=dev)
    used[kept.reshape(-1)] = True
    new = torch.cumsum(used, 0, dtype=torch.int32) - 1
    new = torch.where(used, new, torch.full_like(new, -1))
    sel = torch.nonzero(used).reshape(-1)
    g = lambda t: None if t is None else t[sel]
    out = Mesh(pos[sel], new[kept].to(torch.int32), g(nrm), g(col))
    info = dict(keys=c["keys"], cluster_keys=c["ckeys"], rank=c["rank"], used=used, lo=lo, cell=cell, n=n)
    return out, new[c["rank"].to(torch.int64)], face_map.to(torch.int32), flags[sel], info


def _bisect_cell(v, f, target, origin, dev):
    """the cell of the largest m found whose face count is <= target; cell = bbox diagonal / m"""
    ext = v.amax(0).to(torch.float64) - v.amin(0).to(torch.float64)
    diag = float(torch.sqrt((ext * ext).sum()))
    if not diag > 0.0:
        raise ValueError("target_faces needs a mesh with a positive bounding-box diagonal")

    def count(m):
        try:
            lo, cell, n = _cells(v, diag / m, origin)
            return _count_faces(v, f, lo, cell, n, dev)
        except ValueError:  # more clusters than the face keys hold: finer than anything we can build
            return None

    good, m = None, 1
    bad = None
    while m <= 1 << 20:
        k = count(m)
        if k is None or k > target:
            bad = m
            break
        good = m
        m *= 2
    if good is None:
        raise ValueError(f"target_faces = {target} is not reached even with a single cell over the mesh")
    while bad is not None and bad - good > 1:
        mid = (good + bad) // 2
        k = count(mid)
        if k is not None and k <= target:
            good = mid
        else:
            bad = mid
    return diag / good


def simplify_mesh(mesh, cell=None, target_faces=None, origin=None, lam=1e-3, return_info=False):
    """Quadric vertex clustering (Lindstrom 2000 on Rossignac-Borrel cells): (Mesh, vertex_map int32 [V], face_map int32
    [F'], flags uint8 [V']).  mesh: a Mesh (normals and colours are averaged per cluster, normals renormalised) or
    (vertices, faces).

    All vertices that fall into one cube of side `cell` (an fp32 scalar; the grid starts at `origin`, by default the
    vertex minimum) become ONE vertex, placed where the summed plane quadrics of the cluster's faces are smallest - on a
    plane, a crease or a corner when the cluster holds one - regularised towards the cluster's mean by lam (a convention:
    condition number about 1 / lam), and replaced by the mean when the minimum leaves the cell (flags = 1; flags = 2: the
    cluster has only zero-area faces).  A face survives unless two of its corners merge; of several faces on the same three
    clusters the lowest index survives; survivors keep their order and winding.  The output holds exactly the clusters
    a surviving face uses, in ascending key order.  vertex_map takes an old vertex to its new one (-1: its cluster has
    no surviving face), face_map a new face to its old one.

    Give exactly one of cell and target_faces.  target_faces = n bisects the integer m of cell = bbox diagonal / m with
    count-only passes (keys, ranks and the face remap, no solve) and takes the largest m FOUND whose face count is <= n.
    The only promise is that bound: the face count is not monotone in m (a shifted cell wall can merge what a coarser grid
    kept apart), so a finer admissible cell may exist.  return_info=True appends a dict with the cell actually used
    ("cell"), "lo", "n", and the per-vertex "keys" and "rank" and per-cluster "cluster_keys".

    The order of every sum is fixed by the input (include/panonerf_hip.h): the same bits on every call.  Topology is not
    preserved; edge_counts reports what happened to it."""
    mesh, dev = _as_mesh(mesh)
    if (cell is None) == (target_faces is None):
        raise ValueError("give exactly one of cell and target_faces")
    lam = float(lam)
    if not (lam >= 0.0 and math.isfinite(lam)):
        raise ValueError(f"lam must be finite and >= 0; got {lam!r}")
    if target_faces is not None and (int(target_faces) != target_faces or target_faces < 0):
        raise ValueError(f"target_faces must be a non-negative integer; got {target_faces!r}")
    if cell is not None and not (float(cell) > 0.0 and math.isfinite(float(cell))):
        raise ValueError(f"cell must be positive and finite; got {cell!r}")
    v, f = mesh.vertices, mesh.faces
    V = int(v.shape[0])
    with torch.no_grad(), torch.cuda.device(dev):
        _check(v, f, V, dev)
        if V == 0:
            e = lambda dt: torch.empty(0, dtype=dt, device=dev)
            out = (Mesh(v, f[:0], mesh.normals, mesh.colors), e(torch.int32), e(torch.int32), e(torch.uint8))
            return out + ({"cell": None if cell is None else float(np.float32(cell))},) if return_info else out
        if cell is None:
            cell = _bisect_cell(v, f, int(target_faces), origin, dev)
        lo, c, n = _cells(v, cell, origin)
        out, vmap, fmap, flags, info = _simplify(mesh, lo, c, n, lam, dev)
    return (out, vmap, fmap, flags, info) if return_info else (out, vmap, fmap, flags)


def edge_counts(faces):
    """{"boundary", "nonmanifold", "inconsistent"} (host ints) of an int [F, 3] device tensor of faces: the undirected
    edges that lie in exactly one face, those in more than two, and the directed edges (a, b) used by more than one face
    (two faces that run through an edge the same way are wound against each other).  torch.sort and unique_consecutive on
    device edge keys; edges from a vertex to itself are ignored.  A closed, consistently wound manifold gives 0, 0, 0."""
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be an [F, 3] tensor; got {getattr(faces, 'shape', type(faces))}")
    dev = _device_of(faces)
    with torch.no_grad(), torch.cuda.device(dev):
        f = faces.detach().to(torch.int64)
        a = f.reshape(-1)
        b = f[:, [1, 2, 0]].reshape(-1)
        ok = a != b
        a, b = a[ok], b[ok]
        if a.numel() == 0:
            return {"boundary": 0, "nonmanifold": 0, "inconsistent": 0}
        base = int(torch.maximum(a.max(), b.max())) + 1
        und = torch.sort(torch.minimum(a, b) * base + torch.maximum(a, b))[0]
        cu = torch.unique_consecutive(und, return_counts=True)[1]
        cd = torch.unique_consecutive(torch.sort(a * base + b)[0], return_counts=True)[1]
        return {"boundary": int((cu == 1).sum()), "nonmanifold": int((cu > 2).sum()), "inconsistent": int((cd > 1).sum())}


def _simplify_args(simplify):
    """simplify: a number (the cell) or a dict of simplify_mesh's keywords (cell / target_faces, origin, lam)"""
    if isinstance(simplify, dict):
        bad = sorted(set(simplify) - {"cell", "target_faces", "origin", "lam"})
        if bad:
            raise ValueError(f"simplify holds {bad}; simplify_mesh takes cell, target_faces, origin and lam")
        return dict(simplify)
    if isinstance(simplify, (int, float, np.integer, np.floating)) and not isinstance(simplify, bool):
        return {"cell": float(simplify)}
    raise ValueError(f"simplify must be a cell size or a dict of simplify_mesh's keywords; got {simplify!r}")


def clean_mesh(vertices, faces, simplify=None, min_component_faces=None):
    """(vertices, faces) after the two steps of export_scene and fused_mesh, in their order: filter_components(min_faces =
    min_component_faces) when that is given, then simplify_mesh(**simplify) when that is (simplify: a cell size, or a dict
    of simplify_mesh's keywords).  Attributes are not carried: the callers query the field again at the new vertices."""
    mesh = Mesh(vertices, faces, None, None)
    if min_component_faces is not None:
        mesh = filter_components(mesh, min_faces=min_component_faces)[0]
    if simplify is not None:
        mesh = simplify_mesh(mesh, **_simplify_args(simplify))[0]
    return mesh.vertices, mesh.faces
