"""Generalized winding numbers of a triangle mesh: a robust inside test, signed distance, and a watertight remesh.

``meshdist`` measures how far a point is from a surface; this module says on which side it lies, for meshes that are not
closed: culled TSDF meshes (``fusion``), clustered ones (``meshops.simplify_mesh``) and soups.  The generalized winding number
(Jacobson et al. 2013) is the sum of the signed solid angles of the triangles as seen from the point, over 4 pi: 1 inside and
0 outside a closed mesh whose faces are wound so that (v1 - v0) x (v2 - v0) points outside - the winding of
``marching_tetrahedra`` and ``fusion`` - and a smooth blend of the two over holes and duplicated faces.

    winding_number(points, vertices, faces, accel, beta)          w [P] fp32
    inside(points, vertices, faces, accel, beta)                  bool [P]: w > 0.5
    signed_distance(points, vertices, faces, max_distance, accel, beta)   closest_point's outputs, distance < 0 inside
    winding_grid(mesh, bounds, resolution, accel, beta)           w on geometry's grid [nx, ny, nz]
    signed_distance_grid(mesh, bounds, resolution, max_distance, accel, beta)
    remesh(mesh, resolution, bounds, level, accel, beta)          marching tetrahedra of winding_grid at `level`

Everything that computes is a HIP kernel of ``pn_winding.hip``: the solid angle of van Oosterom and Strackee in fp64 on
the fp32 inputs, summed by brute force through LDS tiles (accel=None: the exact sum) or by a pre-order walk of
``pn_bvh.hip``'s tree that replaces a node by its dipole - its summed vector area N at its area-weighted centroid g - once
the point is beta times the node's radius away (Barnes-Hut, in the manner of Barill et al. 2018).  Everything runs on the
HIP device under ``torch.no_grad()`` on the current stream; CPU tensors raise, there is no host fallback.
include/panonerf_hip.h, section "winding number", states the contract operation for operation and DESIGN.md 6n discusses it.

Conventions.  accel="bvh" (the default) builds a MeshBVH for the call, accel=<a MeshBVH of this mesh> reuses one - its
dipole moments are computed on first use and kept on that object - and accel=None is the exact sum over all faces.  Unlike
closest_point's, the walk's result is an approximation and depends on the tree: its error falls as beta^-2 (DESIGN.md 6n has
the table; beta = 4 is a convention), and it is the same bits on every call.  A point on the surface takes the principal
value (a face seen from its own plane counts 0): 0.5 on a closed surface.  A point with a coordinate that is not finite gets
NaN, is not inside, and keeps closest_point's "no answer".  A face with an index outside [0, V) or a vertex that is not
finite contributes nothing; a mesh without faces gives 0 everywhere.

Out of scope: higher-order (quadrupole) expansions - measured, they did not lower the maximum error at beta = 2 .. 6;
point-cloud or oriented-point inputs; gradients; exact booleans; tuning (the walk's 24 KB LDS stack caps a compute unit at 6
waves, as it does for the tracer and the distance walk).
"""
import math
import sys

import torch

from . import _lib
from .geometry import Mesh, _placement, _resolution, marching_tetrahedra
from .meshdist import _closest, _grid_query, _number, _points, _points_arg, _reach, _tree
from .meshops import _as_mesh
from .objects import MeshBVH, _check_accel

DEFAULT_BETA = 4.0  # a convention: DESIGN.md 6n has the error it buys


def _beta(beta):
    """beta as the fp32 value the kernel sees"""
    return _number(beta, "beta", 1.0, 1e6, "must be a number in [1, 1e6]")


def _moments(tree, v, f, dev):
    """the dipole rows of a MeshBVH, computed on first use and kept on the object"""
    m = getattr(tree, "_winding_moments", None)
    if m is None:
        m = torch.empty(max(tree.F - 1, 1), 8, dtype=torch.float64, device=dev)
        counters = torch.empty(max(tree.F - 1, 1), dtype=torch.int32, device=dev)
        _lib.call("pn_bvh_moments", tree.F, int(v.shape[0]), v.data_ptr(), f.data_ptr(), tree.nodes.data_ptr(), m.data_ptr(),
                  counters.data_ptr(), _lib.stream(dev))
        tree._winding_moments = m
    return m


def _winding(p, v, f, tree, beta, dev):
    """the launch: tree is what objects._prepare returned (a MeshBVH walks, anything else is the exact sum)"""
    P, V, F = int(p.shape[0]), int(v.shape[0]), int(f.shape[0])
    w = torch.empty(P, dtype=torch.float32, device=dev)
    if P == 0:
        return w
    if not V:
        F = 0  # no vertices: no face is valid
    if isinstance(tree, MeshBVH) and tree.F > 0:
        _lib.call("pn_winding_bvh", P, p.data_ptr(), V, v.data_ptr(), F, f.data_ptr(), tree.nodes.data_ptr(),
                  _moments(tree, v, f, dev).data_ptr(), beta, w.data_ptr(), _lib.stream(dev))
    else:
        _lib.call("pn_winding", P, p.data_ptr(), V, _lib.ptr(v) if V else None, F, _lib.ptr(f) if F else None, w.data_ptr(),
                  _lib.stream(dev))
    return w


def _args(points, vertices, faces, accel, beta):
    _check_accel(accel)
    beta = _beta(beta)
    _points_arg(points)
    mesh, dev = _as_mesh(vertices, faces)
    return _points(points, dev), mesh, dev, beta


def winding_number(points, vertices, faces, accel="bvh", beta=DEFAULT_BETA):
    """The generalized winding number of the mesh (vertices [V, 3] fp32, faces [F, 3] int32) at each of points [P, 3] fp32:
    fp32 [P].  accel=None: the exact sum over all faces; "bvh": a Barnes-Hut walk of a tree built for the call; a MeshBVH
    of this mesh: that tree, whose moments are kept on it.  beta in [1, 1e6]: a node is replaced by its dipole from beta
    times its radius on.  The module docstring has the conventions."""
    p, mesh, dev, beta = _args(points, vertices, faces, accel, beta)
    with torch.no_grad(), torch.cuda.device(dev):
        tree = _tree(mesh, dev, accel, p.shape[0])
        return _winding(p, mesh.vertices, mesh.faces, tree, beta, dev)


def inside(points, vertices, faces, accel="bvh", beta=DEFAULT_BETA):
    """bool [P]: winding_number > 0.5 (False where it is NaN)"""
    return winding_number(points, vertices, faces, accel, beta) > 0.5


def _signed(p, v, f, tree, reach, beta, dev):
    dist, face, closest, bary = _closest(p, v, f, tree, reach, dev)
    neg = _winding(p, v, f, tree, beta, dev) > 0.5
    return torch.where(neg, -dist, dist), face, closest, bary


def signed_distance(points, vertices, faces, max_distance=None, accel="bvh", beta=DEFAULT_BETA):
    """meshdist.closest_point's four outputs (distance [P], face [P] int32, closest [P, 3], bary [P, 2]) with the distance
    negated where inside() holds; one tree serves both queries.  A point without an answer (none within max_distance, no
    faces) keeps face = -1 and an infinite distance, with the sign of its side."""
    reach = _reach(max_distance)
    p, mesh, dev, beta = _args(points, vertices, faces, accel, beta)
    with torch.no_grad(), torch.cuda.device(dev):
        tree = _tree(mesh, dev, accel, p.shape[0])
        return _signed(p, mesh.vertices, mesh.faces, tree, reach, beta, dev)


def _grid(mesh, bounds, resolution, accel, beta, query):
    """query(points [m, 3], v, f, tree, beta, dev) -> [m] on geometry's grid, through meshdist._grid_query"""
    _check_accel(accel)
    beta = _beta(beta)
    res = _resolution(resolution)
    lo, step = _placement(bounds, res)
    mesh, dev = _as_mesh(mesh)
    with torch.no_grad(), torch.cuda.device(dev):
        tree = _tree(mesh, dev, accel)
        return _grid_query(mesh, dev, res, lo, step, tree, lambda p: query(p, mesh.vertices, mesh.faces, tree, beta, dev))


def winding_grid(mesh, bounds, resolution, accel="bvh", beta=DEFAULT_BETA):
    """The winding number at the vertices of geometry's grid: a contiguous fp32 [nx, ny, nz] tensor in density_grid's point
    order (bounds are the inclusive corner vertices).  One tree, built once; 2^20 points per launch."""
    return _grid(mesh, bounds, resolution, accel, beta, _winding)


def signed_distance_grid(mesh, bounds, resolution, max_distance=None, accel="bvh", beta=DEFAULT_BETA):
    """signed_distance's first output on geometry's grid, as meshdist.distance_grid gives the unsigned one: fp32
    [nx, ny, nz], negative inside, infinite (with the sign of the side) where no face lies within max_distance."""
    reach = _reach(max_distance)
    return _grid(mesh, bounds, resolution, accel, beta,
                 lambda p, v, f, tree, beta, dev: _signed(p, v, f, tree, reach, beta, dev)[0])


def remesh(mesh, resolution, bounds=None, level=0.5, accel="bvh", beta=DEFAULT_BETA):
    """A watertight, outward-wound Mesh of what `mesh` encloses: marching_tetrahedra of winding_grid at `level`.  For a
    closed input it is the same solid resampled (every vertex within a cell diagonal of the input surface); for an open or
    broken one - a culled TSDF mesh, a clustered mesh, a soup - the 0.5 level of the winding field closes the holes.
    bounds=None: the box of the vertices grown by two grid steps on every side (needs resolution >= 6 per axis).  The
    result has no normals or colours; it feeds filter_components, simplify_mesh, bake_textures and write_ply as any mesh."""
    level = _number(level, "level", -sys.float_info.max, sys.float_info.max, "must be a finite number", fp32=False)
    _check_accel(accel)
    _beta(beta)
    res = _resolution(resolution)
    m, dev = _as_mesh(mesh)
    if bounds is None:
        if min(res) < 6:
            raise ValueError(f"remesh with bounds=None needs resolution >= 6 per axis; got {res}")
        if not m.vertices.shape[0]:
            raise ValueError("remesh with bounds=None needs a mesh with vertices")
        lo, hi = m.vertices.amin(0).to(torch.float64).tolist(), m.vertices.amax(0).to(torch.float64).tolist()  # a host copy
        if not all(math.isfinite(x) for x in lo + hi):
            raise ValueError("the vertices hold a NaN or an infinity")
        h = [(b - a) / (n - 5) for a, b, n in zip(lo, hi, res)]
        bounds = (tuple(a - 2.0 * s for a, s in zip(lo, h)), tuple(b + 2.0 * s for b, s in zip(hi, h)))
    vol = winding_grid(m, bounds, res, accel, beta)
    verts, faces = marching_tetrahedra(vol, level, bounds)
    return Mesh(verts, faces, None, None)
