"""Distances between surfaces: the closest point of a triangle mesh to arbitrary points, and the scores built on it.

The project exports geometry by two routes (``geometry.extract_mesh``, ``fusion.fused_mesh``) and decimates both
(``meshops.simplify_mesh``); this module says how far one surface is from another.

    closest_point(points, vertices, faces, max_distance, accel)   (distance [P], face [P] int32, closest [P, 3], bary [P, 2])
    sample_surface(mesh, count)                                   (points [count, 3], face [count] int32, bary [count, 2])
    compare_meshes(a, b, samples, thresholds, accel)              accuracy / completeness / Chamfer, RMS, Hausdorff,
                                                                  precision / recall / F-score, normal consistency
    distance_grid(mesh, bounds, resolution, max_distance)         unsigned distance on geometry's grid [nx, ny, nz]

Everything that computes is a HIP kernel of ``pn_meshdist.hip``: the point / triangle distance (Ericson's region
classification in fp64 on the fp32 inputs, read from vertices and faces themselves), a brute-force finder through LDS tiles
and a best-first walk of ``pn_bvh.hip``'s tree with a point / box lower bound, and surface sampling whose choice of face is
integer arithmetic (systematic sampling over int64 area weights; the R2 sequence inside the triangle).  torch does the
running sum of the weights and the fp64 sums of the scores.  Everything runs on the HIP device under ``torch.no_grad()`` on
the current stream; CPU tensors raise, there is no host fallback.  include/panonerf_hip.h, section "mesh distance", states
the contract operation for operation, and DESIGN.md 6m discusses it; two calls on the same input give the same bits.

Conventions.  distance = +inf, face = -1 and zeros in closest and bary mean "no answer": a point with a coordinate that is
not finite, a mesh without faces, or no face within max_distance (inclusive).  Among faces at the same fp64 squared
distance the lowest index wins.  bary = (u, v) as trace_mesh reports it, closest = (1 - u - v) v0 + u v1 + v v2, so a
result feeds the same attribute interpolation a ray hit does.  A face with an index outside [0, V) or a vertex that is not
finite is never found and never sampled.  accel="bvh" (the default: the function is new, and the result is the one of
accel=None) builds a MeshBVH for the call, accel=<a MeshBVH of this mesh> reuses one, accel=None is brute force over all
faces.  The walk's result does not depend on the tree and is the brute-force result wherever every face passes the header's
candidate rule, which the triangle boxes' padding provides for; tests/test_meshdist_cpu.py counts the exceptions (none).

Signed distance is ``winding.signed_distance``: the sign comes from the generalized winding number, which does not need the
closed, consistently wound mesh that angle-weighted pseudo-normals would (culled TSDF meshes are neither).  Out of scope
here: point-cloud (vertex-only) targets; the k nearest faces; gradients; tuning the walk (its 24 KB LDS stack caps a compute
unit at 6 waves, as it does for the tracer).
"""
import math

import numpy as np
import torch

from . import _lib
from .geometry import _placement, _resolution
from .meshops import _as_mesh
from .objects import MeshBVH, _check_accel, _prepare

DEFAULT_SAMPLES = 100_000  # per mesh; a convention
DEFAULT_THRESHOLDS = (0.01, 0.02, 0.05)  # in scene units; a convention
GRID_CHUNK = 1 << 20  # grid points per launch of distance_grid


def _points_arg(points):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be a [P, 3] tensor; got {getattr(points, 'shape', type(points))}")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be torch.float32; got {points.dtype}")


def _points(points, dev=None):
    _points_arg(points)
    if points.device.type != "cuda":
        raise RuntimeError(f"pano_nerf_amd.meshdist runs on a HIP device only (points is on {points.device}); there is no "
                           "CPU fallback")
    if dev is not None and points.device != dev:
        raise RuntimeError(f"the points are on {points.device} but the mesh on {dev}")
    return points.detach().contiguous()


def _number(value, name, lo, hi, message, fp32=True):
    """value, a Python or numpy number (no bool, no tensor), as the fp32 the kernel sees (fp32=False: as given), in [lo, hi]"""
    ok = not isinstance(value, (torch.Tensor, bool)) and isinstance(value, (int, float, np.integer, np.floating))
    x = (float(np.float32(value)) if fp32 else float(value)) if ok else math.nan
    if not lo <= x <= hi:
        raise ValueError(f"{name} {message}; got {value!r}")
    return x


def _reach(max_distance):
    """max_distance as the fp32 value the kernel sees; None: +inf"""
    return math.inf if max_distance is None else _number(max_distance, "max_distance", 0.0, math.inf,
                                                          "must be None or a number >= 0")


def _tree(mesh, dev, accel, wanted=True):
    """what objects._prepare makes of accel for this mesh; None for brute force, or when nothing is asked (wanted)"""
    return _prepare(mesh.vertices, mesh.faces, dev, accel) if accel is not None and wanted else None


def _count(count, name="count"):
    if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or not 0 < count < 1 << 31:
        raise ValueError(f"{name} must be an integer in [1, 2^31); got {count!r}")
    return int(count)


def _closest(p, v, f, tree, reach, dev):
    """the launch: tree is what objects._prepare returned (a MeshBVH walks, anything else is brute force)"""
    P, V, F = int(p.shape[0]), int(v.shape[0]), int(f.shape[0])
    dist = torch.empty(P, dtype=torch.float32, device=dev)
    face = torch.empty(P, dtype=torch.int32, device=dev)
    closest = torch.empty(P, 3, dtype=torch.float32, device=dev)
    bary = torch.empty(P, 2, dtype=torch.float32, device=dev)
    if P == 0:
        return dist, face, closest, bary
    if not V:
        F = 0  # no vertices: nothing to find
    walk = isinstance(tree, MeshBVH) and tree.F > 0
    _lib.call("pn_closest_point_bvh" if walk else "pn_closest_point", P, p.data_ptr(), V, _lib.ptr(v) if V else None, F,
              _lib.ptr(f) if F else None, *((tree.nodes.data_ptr(),) if walk else ()), reach, dist.data_ptr(), face.data_ptr(),
              closest.data_ptr(), bary.data_ptr(), _lib.stream(dev))
    return dist, face, closest, bary


def closest_point(points, vertices, faces, max_distance=None, accel="bvh"):
    """The closest point of the mesh (vertices [V, 3] fp32, faces [F, 3] int32) to each of points [P, 3] fp32: (distance [P]
    fp32, face [P] int32, closest [P, 3] fp32, bary [P, 2] fp32 = (u, v) with closest = (1 - u - v) v0 + u v1 + v v2).
    max_distance (a scalar, inclusive) limits the search; a point without an answer gets distance = +inf, face = -1 and
    zeros.  accel="bvh": a walk of a tree built for the call; a MeshBVH of this mesh: that tree; None: brute force.  The
    module docstring has the conventions."""
    _check_accel(accel)
    reach = _reach(max_distance)
    _points_arg(points)
    mesh, dev = _as_mesh(vertices, faces)
    p = _points(points, dev)
    with torch.no_grad(), torch.cuda.device(dev):
        tree = _tree(mesh, dev, accel, p.shape[0])
        return _closest(p, mesh.vertices, mesh.faces, tree, reach, dev)


def _sample(v, f, count, dev):
    V, F = int(v.shape[0]), int(f.shape[0])
    st = _lib.stream(dev)
    W = 0
    if F and V:
        area = torch.empty(F, dtype=torch.float64, device=dev)
        _lib.call("pn_face_areas", F, V, v.data_ptr(), f.data_ptr(), area.data_ptr(), st)
        largest = area.amax().reshape(1)
        weight = torch.empty(F, dtype=torch.int64, device=dev)
        _lib.call("pn_face_weights", F, area.data_ptr(), largest.data_ptr(), weight.data_ptr(), st)
        cum = torch.cumsum(weight, 0)  # int64: exact
        W = int(cum[-1])  # the host sync
    if W <= 0:
        raise ValueError("the mesh has no face with area: nothing to sample")
    points = torch.empty(count, 3, dtype=torch.float32, device=dev)
    face = torch.empty(count, dtype=torch.int32, device=dev)
    bary = torch.empty(count, 2, dtype=torch.float32, device=dev)
    _lib.call("pn_sample_surface", count, W, F, V, v.data_ptr(), f.data_ptr(), cum.data_ptr(), points.data_ptr(),
              face.data_ptr(), bary.data_ptr(), st)
    return points, face, bary


def sample_surface(mesh, count):
    """count points spread over the surface in proportion to area: (points [count, 3] fp32, face [count] int32, bary
    [count, 2] fp32).  Deterministic and the same on every device: the faces get int64 weights floor(area / largest area x
    2^31), sample i takes the face that holds position floor(i W / count) of their running sum W (systematic sampling:
    every face gets the floor or the ceiling of its share count w / W), and its place inside the face is point i of the R2
    low-discrepancy sequence.  Faces without area (or below 2^-31 of the largest) get none; raises ValueError when no face
    has area.  mesh: a Mesh or (vertices, faces)."""
    count = _count(count)
    mesh, dev = _as_mesh(mesh)
    with torch.no_grad(), torch.cuda.device(dev):
        return _sample(mesh.vertices, mesh.faces, count, dev)


def _face_normals(v, f, face):
    """unit geometric normals (fp64) of the faces `face` (all >= 0); 0 for a face without area"""
    tri = v[f[face.to(torch.int64)].to(torch.int64)].to(torch.float64)
    n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return n / n.norm(dim=1, keepdim=True).clamp_min(1e-300)


def _one_way(pa, fa, a, b, tree_b, dev):
    """distances from samples of a to b, and |n . n'| of each sample's own face and its closest face"""
    dist, face, _, _ = _closest(pa, b.vertices, b.faces, tree_b, math.inf, dev)
    found = face >= 0
    dots = (_face_normals(a.vertices, a.faces, fa[found]) * _face_normals(b.vertices, b.faces, face[found])).sum(1).abs()
    return dist.to(torch.float64), dots


def compare_meshes(a, b, samples=DEFAULT_SAMPLES, thresholds=DEFAULT_THRESHOLDS, accel="bvh"):
    """Surface-to-surface scores of mesh a (the estimate) against mesh b (the reference), from `samples` points drawn on
    each with sample_surface and closest_point queries against the other.  A dict of host floats:

        accuracy            mean distance from the samples of a to b         completeness   the same from b to a
        chamfer             (accuracy + completeness) / 2
        rms_ab, rms_ba      root mean square of the same distances
        hausdorff_ab, hausdorff_ba, hausdorff    their maxima, and the larger of the two (of the samples: a lower bound
                            of the true Hausdorff distance)
        thresholds          the tuple tau given;  precision / recall / fscore: one tuple each, per tau - the share of
                            a's samples within tau of b (<=), the share of b's within tau of a, and 2 p r / (p + r)
                            (0 when both are 0)
        normal_consistency  the mean |n . n'| of the geometric normal of each sample's own face and that of its closest
                            face, over the samples of both directions (unoriented: winding does not count)
        samples             the number of samples per mesh

    Sums are fp64.  The defaults - 100 000 samples per mesh and tau = 0.01, 0.02, 0.05 scene units - are conventions,
    not properties of the data: report them with the scores.  a, b: Mesh objects or (vertices, faces); accel as in
    closest_point ("bvh" builds one tree per mesh; a MeshBVH cannot be given, there are two meshes).  Raises when a mesh
    has no face with area."""
    if accel is not None and not (isinstance(accel, str) and accel == "bvh"):
        _check_accel(accel)
        raise ValueError('compare_meshes takes accel=None or "bvh": it queries two meshes')
    n = _count(samples, "samples")
    try:
        taus = tuple(float(t) for t in thresholds)
    except (TypeError, ValueError):
        raise ValueError(f"thresholds must be a sequence of numbers >= 0; got {thresholds!r}")
    if not all(t >= 0.0 for t in taus):
        raise ValueError(f"thresholds must be a sequence of numbers >= 0; got {thresholds!r}")
    a, dev = _as_mesh(a)
    b, dev_b = _as_mesh(b)
    if dev_b != dev:
        raise RuntimeError(f"the meshes are on {dev} and {dev_b}")
    with torch.no_grad(), torch.cuda.device(dev):
        pa, fa, _ = _sample(a.vertices, a.faces, n, dev)
        pb, fb, _ = _sample(b.vertices, b.faces, n, dev)
        tree_a, tree_b = _tree(a, dev, accel), _tree(b, dev, accel)
        dab, nab = _one_way(pa, fa, a, b, tree_b, dev)
        dba, nba = _one_way(pb, fb, b, a, tree_a, dev)
        tau = torch.tensor(taus, dtype=torch.float64, device=dev)
        # fp64 sums and exact counts on the device, one copy, and every division on the host
        head = torch.stack([dab.sum(), dba.sum(), (dab * dab).sum(), (dba * dba).sum(), dab.amax(), dba.amax(),
                            nab.sum() + nba.sum()])
        within_ab = (dab[None, :] <= tau[:, None]).sum(1).to(torch.float64)
        within_ba = (dba[None, :] <= tau[:, None]).sum(1).to(torch.float64)
        host = torch.cat([head, within_ab, within_ba]).cpu().tolist()
        normals = max(nab.numel() + nba.numel(), 1)
    acc, comp, ms_ab, ms_ba = (x / n for x in host[:4])
    h_ab, h_ba, nc = host[4], host[5], host[6] / normals
    k = len(taus)
    p, r = [x / n for x in host[7:7 + k]], [x / n for x in host[7 + k:7 + 2 * k]]
    return {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "rms_ab": math.sqrt(ms_ab),
            "rms_ba": math.sqrt(ms_ba), "hausdorff_ab": h_ab, "hausdorff_ba": h_ba, "hausdorff": max(h_ab, h_ba),
            "thresholds": taus, "precision": tuple(p), "recall": tuple(r),
            "fscore": tuple(2.0 * x * y / (x + y) if x + y > 0.0 else 0.0 for x, y in zip(p, r)),
            "normal_consistency": nc, "samples": n}


def _grid_query(mesh, dev, res, lo, step, tree, query):
    """query(points [m, 3]) -> [m] on geometry's grid, GRID_CHUNK points at a time; mesh and tree are what query closes over"""
    vol = torch.empty(res, dtype=torch.float32, device=dev)
    n = vol.numel()
    pts = torch.empty(min(n, GRID_CHUNK), 3, dtype=torch.float32, device=dev)
    cov = torch.empty_like(pts)
    for first in range(0, n, GRID_CHUNK):
        m = min(GRID_CHUNK, n - first)
        _lib.call("pn_grid_points", *res, first, m, *lo, *step, 0.0, pts.data_ptr(), cov.data_ptr(), _lib.stream(dev))
        vol.view(-1)[first:first + m] = query(pts[:m])
    return vol


def distance_grid(mesh, bounds, resolution, max_distance=None):
    """The unsigned distance to the mesh at the vertices of geometry's grid: a contiguous fp32 [nx, ny, nz] tensor in
    density_grid's point order ((i ny + j) nz + k; bounds are the inclusive corner vertices), +inf where no face lies within
    max_distance.  Plain composition: pn_grid_points places the points, closest_point (one tree, built once) answers them,
    2^20 at a time."""
    res = _resolution(resolution)
    lo, step = _placement(bounds, res)
    reach = _reach(max_distance)
    mesh, dev = _as_mesh(mesh)
    with torch.no_grad(), torch.cuda.device(dev):
        tree = _tree(mesh, dev, "bvh")
        return _grid_query(mesh, dev, res, lo, step, tree,
                           lambda p: _closest(p, mesh.vertices, mesh.faces, tree, reach, dev)[0])
