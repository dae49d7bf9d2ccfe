"""fp64 numpy restatement of the image-based-lighting formulas of include/panonerf_hip.h (pn_ibl.hip): the GGX prefilter,
the environment-BRDF table and the engine's evaluation.  Written from the formulas; the device's direction and
solid-angle tables and its baked maps come in as arrays.  Sums use numpy's own order: the kernels' fixed order differs
from it by a few fp64 roundings only."""
import numpy as np


def prefilter(probes, dirs, omega, directions, roughness):
    """probes [P, 3, H, W], dirs [H W, 3], omega [H W], directions [K, 3] or [P, K, 3] -> [P, K, 3] fp64."""
    x = np.asarray(probes, np.float64)
    P = x.shape[0]
    L = x.reshape(P, 3, -1)
    d, w = np.asarray(dirs, np.float64), np.asarray(omega, np.float64)
    n = np.asarray(directions, np.float64)
    n = np.broadcast_to(n if n.ndim == 3 else n[None], (P,) + n.shape[-2:])
    alpha = float(roughness) ** 2
    out = np.empty((P, n.shape[1], 3))
    for p in range(P):
        c = n[p, :, 0:1] * d[None, :, 0] + n[p, :, 1:2] * d[None, :, 1] + n[p, :, 2:3] * d[None, :, 2]  # [K, HW]
        c = np.maximum(c, 0.0)
        den = ((1.0 + c) / 2.0) * (alpha * alpha - 1.0) + 1.0
        q = c / (den * den)
        sw = (w[None] * q).sum(-1)
        for ch in range(3):
            out[p, :, ch] = ((L[p, ch] * w)[None] * q).sum(-1) / sw
    return out


def brdf_lut(size, samples):
    """[size, size, 2] fp64 (A, B): row i roughness (i + 1/2) / size, column j NoV (j + 1/2) / size."""
    S, n = int(size), int(samples)
    r = ((np.arange(S) + 0.5) / S)[:, None, None, None]
    mu = ((np.arange(S) + 0.5) / S)[None, :, None, None]
    u = ((np.arange(n) + 0.5) / n)[None, None, :, None]
    phi = ((2.0 * np.pi) * ((np.arange(n) + 0.5) / n))[None, None, None, :]
    alpha = r * r
    k = alpha / 2.0
    a2m1 = alpha * alpha - 1.0
    vx = np.sqrt(1.0 - mu * mu)
    c2 = (1.0 - u) / (1.0 + a2m1 * u)
    NoH, sh = np.sqrt(c2), np.sqrt(1.0 - c2)
    VoH = vx * (sh * np.cos(phi)) + mu * NoH
    NoL = (2.0 * VoH) * NoH - mu
    ok = (NoL > 0.0) & (VoH > 0.0)
    NoL_, VoH_ = np.where(ok, NoL, 1.0), np.where(ok, VoH, 1.0)
    g1l = NoL_ / ((1.0 - k) * NoL_ + k)
    g1v = mu / ((1.0 - k) * mu + k)
    Gv = ((g1l * g1v) * VoH_) / (NoH * mu)
    Fc = np.exp2(-(5.55473 * VoH_ + 6.98316) * VoH_)
    A = np.where(ok, (1.0 - Fc) * Gv, 0.0).sum((-1, -2)) / (float(n) * float(n))
    B = np.where(ok, Fc * Gv, 0.0).sum((-1, -2)) / (float(n) * float(n))
    return np.stack([A, B], -1)


def cube_pos(S, d):
    """direction d [R, 3] -> (face, px, py within the face): the major axis picks the face, ties to the earlier face."""
    d0, d1, d2 = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az = np.abs(d0), np.abs(d1), np.abs(d2)
    isx = (ax >= ay) & (ax >= az)
    isy = ~isx & (ay >= az)
    mj = np.where(isx, ax, np.where(isy, ay, az))
    face = np.where(isx, np.where(d0 > 0, 0, 1), np.where(isy, np.where(d1 > 0, 2, 3), np.where(d2 > 0, 4, 5)))
    s_num = np.choose(face, [-d2, d2, d0, d0, d0, -d0])
    t_num = np.choose(face, [-d1, -d1, d2, -d2, -d1, -d1])
    px = (s_num / mj + 1.0) * (0.5 * S)
    py = (t_num / mj + 1.0) * (0.5 * S)
    return face, px, py


def cube_fetch(strip, d):
    """strip [3, 6 S, S], directions d [R, 3] -> [R, 3]: bilinear around (px - 1/2, py - 1/2), taps clamped within the face."""
    strip = np.asarray(strip, np.float64)
    S = strip.shape[2]
    face, px, py = cube_pos(S, d)
    gx, gy = px - 0.5, py - 0.5
    fx, fy = np.floor(gx), np.floor(gy)
    wx, wy = gx - fx, gy - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.clip(x0 + 1, 0, S - 1), np.clip(y0 + 1, 0, S - 1)
    x0, y0 = np.clip(x0, 0, S - 1), np.clip(y0, 0, S - 1)
    top = face * S
    w00, w01, w10, w11 = (1.0 - wy) * (1.0 - wx), (1.0 - wy) * wx, wy * (1.0 - wx), wy * wx
    out = np.empty((d.shape[0], 3))
    for c in range(3):
        ch = strip[c]
        out[:, c] = ((w00 * ch[top + y0, x0] + w01 * ch[top + y0, x1]) + w10 * ch[top + y1, x0]) + w11 * ch[top + y1, x1]
    return out


def cell(u, top):
    """u clamped to [0, top] -> (cell index in [0, top - 1], weight)."""
    u = np.clip(u, 0.0, float(top))
    i = np.minimum(np.floor(u).astype(np.int64), top - 1)
    return i, u - i


def ibl_shade(specular, irradiance, lut, albedo, normals, viewdirs, roughness, f0=0.04):
    """specular: list of [3, 6 S_l, S_l] levels of one probe, irradiance [3, 6 Si, Si], lut [St, St, 2]; rows [R, 3];
    roughness a float or [R] -> (rgb, diffuse, specular) fp64 [R, 3]."""
    n = np.asarray(normals, np.float64)
    vd = np.asarray(viewdirs, np.float64)
    a = np.asarray(albedo, np.float64)
    R = n.shape[0]
    rough = np.broadcast_to(np.asarray(roughness, np.float32).astype(np.float64).reshape(-1), (R,))
    dn = np.sqrt((vd[:, 0] * vd[:, 0] + vd[:, 1] * vd[:, 1]) + vd[:, 2] * vd[:, 2])
    v = -(vd / dn[:, None])
    nv = (n[:, 0] * v[:, 0] + n[:, 1] * v[:, 1]) + n[:, 2] * v[:, 2]
    NoV = np.maximum(nv, 0.0)
    refl = (2.0 * nv)[:, None] * n - v
    levels = len(specular)
    l0, f = cell(rough * (levels - 1), levels - 1)
    lo, hi = np.zeros((R, 3)), np.zeros((R, 3))
    for l in range(levels - 1):
        m = l0 == l
        if m.any():
            lo[m] = cube_fetch(specular[l], refl[m])
            hi[m] = cube_fetch(specular[l + 1], refl[m])
    light = (1.0 - f)[:, None] * lo + f[:, None] * hi
    E = cube_fetch(irradiance, n)
    t = np.asarray(lut, np.float64)
    S = t.shape[0]
    xi, tx = cell(NoV * S - 0.5, S - 1)
    yi, ty = cell(rough * S - 0.5, S - 1)
    w00, w01, w10, w11 = (1.0 - ty) * (1.0 - tx), (1.0 - ty) * tx, ty * (1.0 - tx), ty * tx
    AB = ((w00[:, None] * t[yi, xi] + w01[:, None] * t[yi, xi + 1]) + w10[:, None] * t[yi + 1, xi]) + w11[:, None] * t[yi + 1, xi + 1]
    scale = float(np.float32(f0)) * AB[:, 0] + AB[:, 1]
    diffuse = a / np.pi * E
    spec = light * scale[:, None]
    return diffuse + spec, diffuse, spec


def ulp_ok(got, ref):
    """|got - ref| <= one fp32 unit in the last place of |ref|, element-wise -> (all ok, worst |got - ref| / ulp)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    ratio = np.abs(got - ref) / ulp
    return bool((ratio <= 1.0).all()), float(ratio.max())
