"""A plain numpy fp64 restatement of the texture-atlas conventions (include/panonerf_hip.h, "baking the scene into a
texture atlas"): cell choice, corner UVs, texel ownership and barycentrics, the per-texel geometry, the tangent-space
encoding of normals and the 8-bit quantiser.  Written from the stated conventions, not from the kernels; every output is
computed in fp64 on the fp32 inputs and returned in fp64 (`f32()` rounds once, where the kernels round)."""
import math

import numpy as np

MARGIN, DIAG, MIN_CELL, MAX_SIZE = 1, 2, 6, 16384


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def capacity(S, c):
    return 2 * (S // c) ** 2


def cell_size(F, S):
    """the largest c >= MIN_CELL with 2 (S // c)^2 >= F, by trying them all; ValueError when there is none"""
    for c in range(S, MIN_CELL - 1, -1):
        if capacity(S, c) >= F:
            return c
    raise ValueError(f"{S} x {S} texels are too few for {F} faces")


def smallest_size(F):
    """the smallest S whose atlas holds F faces"""
    S = MIN_CELL
    while capacity(S, MIN_CELL) < F:
        S += 1
    return S


def corners(h, c):
    """[3, 2] (x, y) of P0, P1, P2 inside the cell"""
    L = c - 2 * MARGIN - DIAG
    if h == 0:
        return np.array([[1, 1], [1 + L, 1], [1, 1 + L]], np.float64)
    return np.array([[c - 1, c - 1], [c - 1 - L, c - 1], [c - 1, c - 1 - L]], np.float64)


def cell_origin(f, S, c):
    """(x, y) of the cell of face f in atlas texels"""
    n = S // c
    k = f // 2
    return np.array([(k % n) * c, (k // n) * c], np.float64)


def atlas_xy(F, S, c):
    """[F, 3, 2] fp64: the corners in atlas texel coordinates"""
    out = np.zeros((F, 3, 2))
    for f in range(F):
        out[f] = cell_origin(f, S, c) + corners(f & 1, c)
    return out


def atlas_uv(F, S, c):
    """[3F, 2] fp64 (OBJ convention: U = X / S, V = 1 - Y / S)"""
    xy = atlas_xy(F, S, c).reshape(-1, 2)
    return np.stack([xy[:, 0] / S, 1.0 - xy[:, 1] / S], 1)


def owners(S, c, F):
    """face [S, S] int32 (-1 unowned), u, v [S, S] fp64 (0 where unowned)"""
    n = S // c
    L = float(c - 2 * MARGIN - DIAG)
    face = np.full((S, S), -1, np.int32)
    u, v = np.zeros((S, S)), np.zeros((S, S))
    for i in range(S):
        for j in range(S):
            if i >= n * c or j >= n * c:
                continue
            li, lj = i % c, j % c
            h = 1 if li + lj + 1 >= c else 0
            f = 2 * ((i // c) * n + (j // c)) + h
            if f >= F:
                continue
            x, y = lj + 0.5, li + 0.5
            face[i, j] = f
            if h == 0:
                u[i, j], v[i, j] = (x - 1) / L, (y - 1) / L
            else:
                u[i, j], v[i, j] = (c - 1 - x) / L, (c - 1 - y) / L
    return face, u, v


def texels(S, c, vertices, faces, vnormals=None):
    """dict of fp64 arrays: face [S, S] int32, bary [S, S, 2], points, normals_g, normals_s [S, S, 3], var [S, S]"""
    V64 = np.asarray(vertices, np.float32).astype(np.float64)
    faces = np.asarray(faces)
    F, V = len(faces), len(V64)
    L = float(c - 2 * MARGIN - DIAG)
    face, u, v = owners(S, c, F)
    out = dict(face=face, bary=np.zeros((S, S, 2)), points=np.zeros((S, S, 3)), normals_g=np.zeros((S, S, 3)),
               normals_s=np.zeros((S, S, 3)), var=np.zeros((S, S)))
    for i in range(S):
        for j in range(S):
            f = face[i, j]
            if f < 0:
                continue
            idx = [int(q) for q in faces[f]]
            if not all(0 <= q < V for q in idx):
                continue
            p0, p1, p2 = (V64[q] for q in idx)
            if not (np.isfinite(p0).all() and np.isfinite(p1).all() and np.isfinite(p2).all()):
                continue
            uu, vv = u[i, j], v[i, j]
            w0 = 1.0 - uu - vv
            out["bary"][i, j] = (uu, vv)
            out["points"][i, j] = w0 * p0 + uu * p1 + vv * p2
            g = np.cross(p1 - p0, p2 - p0)
            A_w = math.sqrt(float(g @ g))
            if A_w == 0.0:
                continue
            out["var"][i, j] = A_w / (12.0 * L * L)
            out["normals_g"][i, j] = g / A_w
            if vnormals is None:
                out["normals_s"][i, j] = f32(g / A_w)  # the same fp32 values as normals_g
            else:
                n0, n1, n2 = (np.asarray(vnormals, np.float32)[q].astype(np.float64) for q in idx)
                b = w0 * n0 + uu * n1 + vv * n2
                out["normals_s"][i, j] = b / max(math.sqrt(float(b @ b)), 1e-30)
    return out


def _unit(v):
    n = math.sqrt(float(v @ v))
    return v / n if n >= 1e-12 else None


def encode_normals(S, vertices, faces, uv, face, normals_s, world):
    """[S, S, 3] fp64: 0.5 m + 0.5 in the Gram-Schmidt frame of the sampler (the header's "Normal map"), (0.5, 0.5, 1) where
    the frame does not exist, the face is nobody's, or the normal faces away from N"""
    V64 = np.asarray(vertices, np.float32).astype(np.float64)
    uv64 = np.asarray(uv, np.float32).astype(np.float64)
    faces = np.asarray(faces)
    F, V = len(faces), len(V64)
    out = np.empty((S, S, 3))
    out[...] = (0.5, 0.5, 1.0)
    Ns = np.asarray(normals_s, np.float32).astype(np.float64)
    W = np.asarray(world, np.float32).astype(np.float64)
    for i in range(S):
        for j in range(S):
            f = int(face[i, j])
            if not 0 <= f < F:
                continue
            idx = [int(q) for q in faces[f]]
            if not all(0 <= q < V for q in idx):
                continue
            p0, p1, p2 = (V64[q] for q in idx)
            q0, q1, q2 = uv64[3 * f], uv64[3 * f + 1], uv64[3 * f + 2]
            with np.errstate(all="ignore"):
                e1, e2 = p1 - p0, p2 - p0
                du1, dv1 = q1 - q0
                du2, dv2 = q2 - q0
                det = float(du1 * dv2 - du2 * dv1)
                if det == 0.0 or not math.isfinite(det):
                    continue
                N, n = Ns[i, j], W[i, j]
                T = (e1 * dv2 - e2 * dv1) / det
                B = (e2 * du1 - e1 * du2) / det
                Tn = _unit(T - N * float(N @ T))
                if Tn is None or not np.isfinite(Tn).all():
                    continue
                Bn = _unit(B - N * float(N @ B) - Tn * float(Tn @ B))
                if Bn is None or not np.isfinite(Bn).all():
                    continue
                m = np.array([float(n @ Tn), float(n @ Bn), float(n @ N)])
            if not np.isfinite(m).all() or not m[2] > 0.0:
                continue
            out[i, j] = 0.5 * m + 0.5
    return out


def quantize(x, table=None):
    """uint8 of fp32 x: the nearest code by a binary search of the increasing table (ties to the lower code), or
    round-half-even(255 clamp(x)); NaN gives 0"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(x > 0, np.minimum(x, np.float32(1.0)), np.float32(0.0)).astype(np.float64)  # NaN -> 0
    if table is None:
        return np.rint(255.0 * v).astype(np.uint8)  # numpy's rint rounds half to even
    t = np.asarray(table, np.float32).astype(np.float64)
    lo = np.clip(np.searchsorted(t, v, side="right") - 1, 0, 255)
    hi = np.minimum(lo + 1, 255)
    return np.where(t[hi] - v < v - t[lo], hi, lo).astype(np.uint8)


def quantize_brute(x, table):
    """the same by brute force: argmin over all 256 codes of |table[i] - clamp(x)| in fp64 (argmin keeps the first = lower)"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(x > 0, np.minimum(x, np.float32(1.0)), np.float32(0.0)).astype(np.float64)
    t = np.asarray(table, np.float32).astype(np.float64)
    return np.argmin(np.abs(t[None, :] - v.reshape(-1, 1)), axis=1).astype(np.uint8).reshape(x.shape)

