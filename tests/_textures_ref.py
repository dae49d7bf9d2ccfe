"""A plain numpy restatement of the texture conventions (include/panonerf_hip.h, "texture-mapped materials"): decode
tables, the fp32 mip pyramid, and - in fp64, row by row - UV interpolation, the ray-cone level of detail, bilinear and
trilinear filtering and the tangent-space normal map.  Written from the stated conventions, not from the kernels; it is
slow on purpose (python loops over rows) and is meant for a few hundred rows."""
import math

import numpy as np


def decode_table(srgb):
    """256 fp32 values: i / 255, or the sRGB EOTF of it; built in fp64 and rounded once."""
    c = np.arange(256, dtype=np.float64) / 255.0
    if srgb:
        c = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    return c.astype(np.float32)


def num_levels(H, W):
    return 1 + int(math.floor(math.log2(max(H, W))))


def level_shapes(H, W):
    """[(texel offset, h_l, w_l)] of the concatenated pyramid"""
    out, off = [], 0
    for l in range(num_levels(H, W)):
        h, w = max(1, H >> l), max(1, W >> l)
        out.append((off, h, w))
        off += h * w
    return out


def level0(image, srgb=False):
    """uint8 or fp32 [H, W] / [H, W, C] -> fp32 [H, W, 4]: unused channels 0, alpha 1"""
    img = np.asarray(image)
    if img.ndim == 2:
        img = img[:, :, None]
    H, W, C = img.shape
    out = np.zeros((H, W, 4), np.float32)
    out[..., 3] = 1.0
    if img.dtype == np.uint8:
        tab = decode_table(srgb)
        for c in range(C):
            out[..., c] = (img[..., c].astype(np.float64) / 255.0).astype(np.float32) if c == 3 else tab[img[..., c]]
    else:
        out[..., :C] = img.astype(np.float32)
    return out


def pyramid(lvl0):
    """[H, W, 4] fp32 -> list of levels, each ((a + b) + (c + d)) * 0.25f in fp32 with clamped source rows / columns"""
    levels = [np.asarray(lvl0, np.float32)]
    H, W = levels[0].shape[:2]
    for l in range(num_levels(H, W) - 1):
        s = levels[-1]
        hs, ws = s.shape[:2]
        hd, wd = max(1, H >> (l + 1)), max(1, W >> (l + 1))
        y, x = np.arange(hd), np.arange(wd)
        r0, r1 = np.minimum(2 * y, hs - 1), np.minimum(2 * y + 1, hs - 1)
        c0, c1 = np.minimum(2 * x, ws - 1), np.minimum(2 * x + 1, ws - 1)
        a, b = s[r0][:, c0], s[r0][:, c1]
        c, d = s[r1][:, c0], s[r1][:, c1]
        levels.append(((a + b) + (c + d)) * np.float32(0.25))
        assert levels[-1].dtype == np.float32
    return levels


def flat_pyramid(levels):
    return np.concatenate([l.reshape(-1, 4) for l in levels], 0)


def _index(i, n, wrap):
    i = int(i)
    return min(max(i, 0), n - 1) if wrap == "clamp" else i % n  # python's % is the non-negative modulo


def bilinear(level, U, V, wrap):
    """level [h, w, 4] -> 4 fp64 values at (U, V) (V already flipped)"""
    h, w = level.shape[:2]
    x, y = U * w - 0.5, V * h - 0.5
    x0, y0 = math.floor(x), math.floor(y)
    fx, fy = x - x0, y - y0
    xa, xb, ya, yb = _index(x0, w, wrap), _index(x0 + 1, w, wrap), _index(y0, h, wrap), _index(y0 + 1, h, wrap)
    a00, a01, a10, a11 = (level[j, i].astype(np.float64) for j, i in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
    return (1 - fy) * ((1 - fx) * a00 + fx * a01) + fy * ((1 - fx) * a10 + fx * a11)


def trilinear(levels, lam, U, V, wrap):
    L = len(levels)
    l0 = int(math.floor(lam))
    f = lam - l0
    l1 = min(l0 + 1, L - 1)
    return (1 - f) * bilinear(levels[l0], U, V, wrap) + f * bilinear(levels[l1], U, V, wrap)


def _log2(x):
    if x != x:
        return float("nan")
    if x == 0:
        return float("-inf")
    if x < 0:
        return float("nan")
    return math.log2(x) if x != float("inf") else float("inf")


def lod(H, W, A_uv, A_w, width, c):
    """the clamped level of detail lambda of an H x W texture (fp64)"""
    with np.errstate(all="ignore"):
        ratio = float(np.float64(W) * np.float64(H) * np.float64(A_uv) / np.float64(A_w))
    lam = 0.5 * _log2(ratio) + _log2(width) - _log2(c)
    top = num_levels(H, W) - 1
    if lam != lam:
        return 0.0
    return min(max(lam, 0.0), float(top))


def _unit(v):
    n = math.sqrt(float(v @ v))
    return (v / n if n >= 1e-12 else None)


def texture_hits(mask, face, bary, directions, t, normals, radii, vertices, faces, uv, face_uv, textures, wrap, flip_v):
    """textures: dict name -> list of levels (names among "albedo", "roughness", "normal").  Returns dict of fp64 arrays:
    albedo [R, 3], roughness [R], normals [R, 3] (each only if its texture is given), lod [R, 3] (albedo, roughness,
    normal; 0 where the texture is absent) and fallback [R] bool (normal map rows that kept N)."""
    R = len(mask)
    V64, uv64 = np.asarray(vertices, np.float64), np.asarray(uv, np.float64)
    out = dict(lod=np.zeros((R, 3)), fallback=np.zeros(R, bool))
    if "albedo" in textures:
        out["albedo"] = np.zeros((R, 3))
    if "roughness" in textures:
        out["roughness"] = np.zeros(R)
    if "normal" in textures:
        out["normals"] = np.zeros((R, 3))
    order = ("albedo", "roughness", "normal")
    for r in range(R):
        if not mask[r]:
            continue
        f = int(face[r])
        i0, i1, i2 = (int(i) for i in faces[f])
        js = [int(j) for j in (face_uv[f] if face_uv is not None else faces[f])]
        if all(0 <= j < len(uv64) for j in js):
            q0, q1, q2 = (uv64[j] for j in js)
        else:
            q0 = q1 = q2 = np.array([np.nan, np.nan])
        u, v = float(bary[r][0]), float(bary[r][1])
        w0 = 1.0 - u - v
        with np.errstate(all="ignore"):
            UV = w0 * q0 + u * q1 + v * q2
            du1, dv1 = q1 - q0
            du2, dv2 = q2 - q0
            det = float(du1 * dv2 - du2 * dv1)
        U, Vc = float(UV[0]), float(UV[1])
        finite = math.isfinite(U) and math.isfinite(Vc)
        Vs = 1.0 - Vc if flip_v else Vc
        e1, e2 = V64[i1] - V64[i0], V64[i2] - V64[i0]
        d = np.asarray(directions[r], np.float64)
        g = np.cross(e1, e2)
        A_w = math.sqrt(float(g @ g))
        with np.errstate(all="ignore"):
            c = abs(float((g / A_w) @ d)) / math.sqrt(float(d @ d))
        width = 2.0 * float(radii[r]) * float(t[r]) if radii is not None else 0.0
        N = np.asarray(normals[r], np.float64)
        for k, name in enumerate(order):
            if name not in textures:
                continue
            levels = textures[name]
            H, W = levels[0].shape[:2]
            lam = lod(H, W, abs(det), A_w, width, c)
            out["lod"][r, k] = lam
            s = trilinear(levels, lam, U, Vs, wrap)[:3] if finite else np.zeros(3)
            if name == "albedo":
                out["albedo"][r] = s
            elif name == "roughness":
                out["roughness"][r] = s[0]
            else:
                n = None
                if finite and det != 0.0 and math.isfinite(det):
                    m = 2.0 * s - 1.0
                    T = (e1 * dv2 - e2 * dv1) / det
                    B = (e2 * du1 - e1 * du2) / det
                    Tn = _unit(T - N * float(N @ T))
                    if Tn is not None:
                        Bn = _unit(B - N * float(N @ B) - Tn * float(Tn @ B))
                        if Bn is not None:
                            n = _unit(m[0] * Tn + m[1] * Bn + m[2] * N)
                    if n is not None and not (np.isfinite(n).all() and float(n @ d) < 0.0):
                        n = None
                out["fallback"][r] = n is None
                out["normals"][r] = N if n is None else n
    return out
