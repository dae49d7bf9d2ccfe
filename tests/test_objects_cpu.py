"""fp64 numpy restatement of the object-insertion contract (include/panonerf_hip.h, pano_nerf_amd.objects): the
Moeller-Trumbore tracer with its edge rule and tie-break, the reference's Lambertian / microfacet shading under light
probes, the differential shadow ratio, hit attributes and the composite.  Checked here against the reference's own
outputs (tests/golden/objects_ref.npz) and analytic cases, together with geometry.read_ply and the argument checks that
need no device; test_gpu_objects.py checks the kernels against it."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import load_golden, rel_err

_spec = importlib.util.spec_from_file_location("_lighting_spec_for_objects",
                                               os.path.join(os.path.dirname(__file__), "test_lighting_cpu.py"))
lspec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lspec)

EDGE_EPS = float(np.float32(2e-6))  # PN_OBJ_EDGE_EPS


# ------------------------------------------------------------------------------------------------------------ meshes
def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """(vertices [V, 3] fp32, faces [20 4^level, 3] int32) of a subdivided icosahedron, vertices on the sphere (fp64,
    rounded once), faces wound outwards."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1),
         (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = np.array(v) * radius + np.asarray(centre, dtype=np.float64)
    return verts.astype(np.float32), np.array(f, dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------ tracer
def trace(origins, directions, vertices, faces, t_max=None, dtype=np.float64, margin=None, chunk=2048):
    """Closest hit per ray, the kernel's rule in `dtype` arithmetic: p = d x e2, det = e1 . p, inv = 1 / det, s = o - v0,
    u = (s . p) inv, q = s x e1, v = (d . q) inv, t = (e2 . q) inv; hit when det != 0, u >= -eps, v >= -eps,
    u + v <= 1 + eps, 0 < t < inf (and t < t_max); the lowest face index among equal t.
    -> (t [R] (+inf), face [R] (-1), bary [R, 2]) and, with `margin`, near [R] bool: some triangle in front of the ray
    (t > 0) has min(|u|, |v|, |1 - u - v|) < margin."""
    o, d = np.asarray(origins, dtype), np.asarray(directions, dtype)
    vt, fc = np.asarray(vertices, dtype), np.asarray(faces, np.int64)
    R, F = o.shape[0], fc.shape[0]
    T = np.full(R, np.inf, dtype)
    Fi = np.full(R, -1, np.int32)
    B = np.zeros((R, 2), dtype)
    near = np.zeros(R, bool)
    if not F or not R:
        return (T, Fi, B) + ((near,) if margin is not None else ())
    v0 = vt[fc[:, 0]]
    e1, e2 = vt[fc[:, 1]] - v0, vt[fc[:, 2]] - v0
    eps, one = dtype(EDGE_EPS), dtype(1)
    dot = lambda a, b: a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]
    cross = lambda a, b: np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                   a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    for first in range(0, R, chunk):
        sl = slice(first, min(first + chunk, R))
        oo, dd = o[sl, None, :], d[sl, None, :]
        with np.errstate(all="ignore"):
            p = cross(dd, e2[None])
            det = dot(e1[None], p)
            inv = one / det
            s = oo - v0[None]
            u = dot(s, p) * inv
            q = cross(s, e1[None])
            v = dot(dd, q) * inv
            t = dot(e2[None], q) * inv
            front = (det != 0) & (t > 0) & (t < np.inf)
            hit = front & (u >= -eps) & (v >= -eps) & (u + v <= one + eps)
            if t_max is not None:
                hit &= t < np.asarray(t_max, dtype)[sl, None]
            if margin is not None:
                m = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(one - u - v))
                near[sl] = (front & (m < margin)).any(1)
        tt = np.where(hit, t, np.inf)
        j = np.argmin(tt, 1)  # the first minimum: the lowest face index among equal t
        r = np.arange(tt.shape[0])
        ok = hit[r, j]
        T[sl] = np.where(ok, tt[r, j], np.inf)
        Fi[sl] = np.where(ok, j, -1)
        B[sl, 0], B[sl, 1] = np.where(ok, u[r, j], 0), np.where(ok, v[r, j], 0)
    return (T, Fi, B) + ((near,) if margin is not None else ())


def pano_rays(H, W, origin):
    """(origins, unit directions) [H W, 3] fp64 of an identity-rotation equirectangular camera at `origin`."""
    d = lspec.probe_dirs(H, W)
    return np.broadcast_to(np.asarray(origin, np.float64), d.shape).copy(), d


def look_at(eye, target, up=(0, 1, 0)):
    e, t, u = (np.asarray(x, np.float64) for x in (eye, target, up))
    z = (e - t) / np.linalg.norm(e - t)
    x = np.cross(u, z)
    x /= np.linalg.norm(x)
    out = np.eye(4)
    out[:3, :4] = np.stack([x, np.cross(z, x), z, e], 1)
    return out


def pinhole_rays(H, W, fov_x_deg, c2w):
    """(origins, directions) [H W, 3] fp64: ((j + .5 - W/2) / f, -(i + .5 - H/2) / f, -1) rotated, NOT normalised."""
    f = 0.5 * W / np.tan(0.5 * np.radians(fov_x_deg))
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    cam = np.stack([(j + 0.5 - W / 2) / f, -(i + 0.5 - H / 2) / f, -np.ones_like(j)], -1).reshape(-1, 3)
    d = cam @ c2w[:3, :3].T
    return np.broadcast_to(c2w[:3, 3], d.shape).copy(), d


def line_distance(o, d, c):
    """(distance of the line o + t d from c, t of the closest point)."""
    m = np.asarray(c, np.float64) - o
    dd = (d * d).sum(-1)
    tc = (m * d).sum(-1) / dd
    return np.linalg.norm(m - tc[:, None] * d, axis=-1), tc


# ------------------------------------------------------------------------------------------------------------ shading
def shade(probes, dirs, omega, albedo, normals, viewdirs, roughness=None, weights=None):
    """probes [K, HW, 3]; -> (rgb, diffuse, specular, shading | None) [R, 3] fp64: surface_rendering /
    surface_rendering_wlit with the probe pixels as lights and v = -viewdirs, under the light sum_k weights[r, k] L_k."""
    L = np.asarray(probes, np.float64)
    l, om = np.asarray(dirs, np.float64), np.asarray(omega, np.float64)
    a, n = np.asarray(albedo, np.float64), np.asarray(normals, np.float64)
    v = -np.asarray(viewdirs, np.float64)
    R = a.shape[0]
    w = np.ones((R, 1)) if weights is None else np.asarray(weights, np.float64)
    Lw = np.einsum("rk,kpc->rpc", w, L) * om[None, :, None]  # [R, HW, 3]
    with np.errstate(all="ignore"):
        NoL = np.maximum(n @ l.T, 0.0)  # [R, HW]
        shading = (Lw * NoL[..., None]).sum(1)
        diffuse = a / np.pi * shading
        if roughness is None:
            return diffuse, diffuse, np.zeros_like(diffuse), shading
        r = np.broadcast_to(np.asarray(roughness, np.float64).reshape(-1, 1), (R, 1))
        h = l[None] + v[:, None]
        h = h / np.maximum(np.linalg.norm(h, axis=-1, keepdims=True), 1e-12)
        NoH = np.maximum((n[:, None] * h).sum(-1), 0.0)
        VoH = np.maximum((v[:, None] * h).sum(-1), 0.0)
        NoV = np.maximum((n * v).sum(-1, keepdims=True), 0.0)
        alpha, k = r ** 2, r ** 2 / 2
        D = alpha ** 2 / (np.pi * ((NoH ** 2) * (alpha ** 2 - 1) + 1) ** 2)
        Fr = 0.04 + (1 - 0.04) * 2.0 ** (-(5.55473 * VoH + 6.98316) * VoH)
        G = NoL / ((1 - k) * NoL + k) * (NoV / ((1 - k) * NoV + k))
        sp = D * Fr * G / (4 * NoL * NoV)
        sp = np.where(np.isnan(sp) | (sp == np.inf), 0.0, sp)
        specular = (sp[..., None] * Lw).sum(1)
    return diffuse + specular, diffuse, specular, None


# ------------------------------------------------------------------------------------------------------------ shadows
def shadow_ratio(points, normals, probe, dirs, omega, vertices, faces, bias=1e-3, margin=1e-5):
    """probe [HW, 3], dirs [HW, 3] (the table the kernel reads), omega [HW]; -> (ratio [R] fp64, margin_share [R]: the
    share of E(all) carried by (point, pixel) pairs whose shadow ray passes within `margin` (barycentric) of an edge of a
    triangle in front of it, n_pairs).  The shadow-ray origin is the kernel's: fl(x + fl(bias n)), widened."""
    x32, n32 = np.asarray(points, np.float32), np.asarray(normals, np.float32)
    with np.errstate(all="ignore"):
        o = (x32 + np.float32(bias) * n32).astype(np.float64)
    n = n32.astype(np.float64)
    l = np.asarray(dirs, np.float64)
    wpix = np.asarray(probe, np.float64).mean(-1) * np.asarray(omega, np.float64)
    R = o.shape[0]
    ok = np.isfinite(x32).all(1) & np.isfinite(n32).all(1)
    with np.errstate(all="ignore"):
        c = n @ l.T
    wgt = np.where(c > 0, wpix[None] * c, 0.0)
    e_all = wgt.sum(1)
    occ = np.zeros(c.shape, bool)
    near = np.zeros(c.shape, bool)
    pairs = 0
    if len(faces):
        vt = np.asarray(vertices, np.float64)
        centre = (vt.min(0) + vt.max(0)) / 2
        rad = np.linalg.norm(vt - centre, axis=1).max() * 1.05 + 1e-6
        rr, pp = np.nonzero((c > 0) & ok[:, None])
        dist, tc = line_distance(o[rr], l[pp], centre)
        inside = np.linalg.norm(o[rr] - centre, axis=1) <= rad
        keep = (dist <= rad) & ((tc > 0) | inside)
        rr, pp = rr[keep], pp[keep]
        pairs = rr.size
        t, _, _, nr = trace(o[rr], l[pp], vertices, faces, margin=margin)
        occ[rr, pp] = np.isfinite(t)
        near[rr, pp] = nr
    e_un = np.where(occ, 0.0, wgt).sum(1)
    with np.errstate(all="ignore"):
        ratio = np.where(ok & (e_all > 0), np.clip(e_un / e_all, 0.0, 1.0), 1.0)
        share = np.where(e_all > 0, np.where(near, wgt, 0.0).sum(1) / e_all, 0.0)
    return ratio, share, pairs


# ----------------------------------------------------------------------------------------------------- hit attributes
def hit_attributes(origins, directions, t, face, bary, vertices, faces, vnormals=None, albedo=(0.8, 0.8, 0.8),
                   scene_dep=None, probe_positions=None):
    """dict of fp64 arrays: mask, points, normals, albedo, viewdirs, weights, scene_points - the kernel's rules."""
    o, d = np.asarray(origins, np.float64), np.asarray(directions, np.float64)
    t, face = np.asarray(t, np.float64), np.asarray(face, np.int64)
    vt, fc = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    mask = face >= 0
    with np.errstate(all="ignore"):
        if scene_dep is not None:
            mask &= ~(t >= np.asarray(scene_dep, np.float64))
        f = np.where(mask, face, 0)
        i0, i1, i2 = fc[f, 0], fc[f, 1], fc[f, 2]
        u, v = np.asarray(bary, np.float64)[:, 0:1], np.asarray(bary, np.float64)[:, 1:2]
        w0 = 1.0 - u - v
        pts = o + np.where(mask, t, 0.0)[:, None] * d
        wdir = d / np.linalg.norm(d, axis=1, keepdims=True)
        if vnormals is not None:
            vn = np.asarray(vnormals, np.float64)
            n = w0 * vn[i0] + u * vn[i1] + v * vn[i2]
        else:
            n = np.cross(vt[i1] - vt[i0], vt[i2] - vt[i0])
        n = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
        n = np.where((n * wdir).sum(1, keepdims=True) > 0, -n, n)
        alb = np.asarray(albedo, np.float64)
        a = (w0 * alb[i0] + u * alb[i1] + v * alb[i2]) if alb.ndim == 2 else np.broadcast_to(alb, pts.shape)
        z = lambda x: np.where(mask[:, None], x, 0.0)
        out = dict(mask=mask, points=z(pts), normals=z(n), albedo=z(a), viewdirs=z(wdir))
        if scene_dep is not None:
            sp = o + np.asarray(scene_dep, np.float64).reshape(-1, 1) * d
            out["scene_points"] = np.where(mask[:, None], np.nan, sp)
        if probe_positions is not None:
            dist = np.linalg.norm(pts[:, None] - np.asarray(probe_positions, np.float64)[None], axis=-1)
            exact = dist <= 1e-6
            inv = np.where(exact, 0.0, 1.0 / dist)
            w = inv / inv.sum(1, keepdims=True)
            first = np.zeros_like(w)
            first[np.arange(len(w)), exact.argmax(1)] = 1.0
            w = np.where(exact.any(1, keepdims=True), first, w)
            out["weights"] = z(w)
    return out


def composite(mask, object_rgb, t, scene_rgb, scene_dep, shadow):
    m = np.asarray(mask, bool)
    return np.where(m[:, None], object_rgb, scene_rgb * shadow[:, None]), np.where(m, t, scene_dep)


# ------------------------------------------------------------------------------------------------------ tests: goldens
def _case(g, size):
    H, W = (int(s) for s in size.split("x"))
    k = size + "/"
    # the reference's fp64 run takes the fp32 direction table widened and the unrounded solid angles
    return k, g[k + "probes"], g[k + "dirs"], lspec.probe_omega(H, W)


@pytest.mark.parametrize("size", ["16x32", "32x64"])
def test_restatement_is_the_reference_shading(size):
    g = load_golden("objects_ref")
    k, probes, dirs, omega = _case(g, size)
    a, n, vd = g[k + "albedo"], g[k + "normal"], -g[k + "v"]
    got = shade(probes[:1], dirs, omega, a, n, vd)
    for name, x in zip(("rgb", "diffuse", "specular", "shading"), got):
        e = rel_err(x, g[k + "lambert/" + name + "64"])
        print(size, "lambert", name, e)
        assert e < 1e-6 or not np.abs(g[k + "lambert/" + name + "64"]).max(), (name, e)
    got = shade(probes[:1], dirs, omega, a, n, vd, g[k + "micro_hi/roughness"])
    for name, x in zip(("rgb", "diffuse", "specular"), got):
        e = rel_err(x, g[k + "micro_hi/" + name + "64"])
        print(size, "micro_hi", name, e)
        assert e < 1e-6, (name, e)
    got = shade(probes[:1], dirs, omega, a, n, vd, g[k + "micro_lo/roughness"])
    for name, x in zip(("rgb", "diffuse", "specular"), got):
        e = rel_err(x, g[k + "micro_lo/" + name + "64"])
        print(size, "micro_lo", name, e)
        assert e < 1e-6, (name, e)
    # K = 3 through surface_rendering_wlit: only an fp32 run of it exists (it asserts roughness is None and is linear in
    # the light).  Its own rounding: three fp32 products per term and torch's pairwise fp32 sums over H W <= 2048 terms,
    # (3 + log2(2048)) x 2^-24 ~ 8e-7 relative to the sum of magnitudes, which for these non-negative terms is the sum
    got = shade(probes, dirs, omega, a, n, vd, None, g[k + "weights"])
    for name, x in zip(("rgb", "diffuse", "specular", "shading"), got):
        ref = g[k + "lambert_k3/" + name]
        e = rel_err(x, ref)
        print(size, "lambert_k3", name, e)
        assert e < 2e-6 or not np.abs(ref).max(), (name, e)


def test_shading_edge_rows_are_finite():
    rng = np.random.default_rng(5)
    H, W = 8, 16
    dirs, omega = lspec.probe_dirs(H, W), lspec.probe_omega(H, W)
    probes = rng.random((1, H * W, 3))
    n = np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    vd = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])  # grazing (NoV = 0) and from behind (NoV clamped to 0)
    rgb, diffuse, specular, _ = shade(probes, dirs, omega, np.ones((2, 3)), n, vd, 0.4)
    assert np.isfinite(rgb).all() and np.all(specular == 0.0) and np.all(diffuse > 0)


# ----------------------------------------------------------------------------------------------------- tests: tracer
def test_tracer_against_analytic_sphere_distances():
    """The icosphere's vertices lie on the sphere of radius r, so the mesh (convex) lies inside the closed ball of radius r
    and contains the ball of radius r_in = min over faces of the distance of the face's plane from the centre
    = r cos(rho), rho the angular radius of the face's circumcircle: r - r_in is the sagitta of the subdivision level.
    A ray from outside whose line meets the inner ball therefore enters the mesh between the two analytic distances."""
    c, r = np.array([0.5, -0.1, 0.8]), 0.35
    for level, sag_bound in ((1, 0.12), (3, 0.008)):
        v, f = icosphere(level, r, c)
        vt = v.astype(np.float64)
        nrm = np.cross(vt[f[:, 1]] - vt[f[:, 0]], vt[f[:, 2]] - vt[f[:, 0]])
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        plane = ((vt[f[:, 0]] - c) * nrm).sum(1)
        assert (plane > 0).all()  # wound outwards
        r_in = plane.min()
        # rho <= the largest vertex-to-centroid angle of a face
        cen = vt[f].mean(1) - c
        cen /= np.linalg.norm(cen, axis=1, keepdims=True)
        rho = np.arccos(np.clip(((vt[f] - c) / r * cen[:, None]).sum(-1), -1, 1)).max()
        assert r - r_in <= r * (1 - np.cos(rho)) * (1 + 1e-6) + 1e-7 and r - r_in < sag_bound * r * 3
        o, d = pano_rays(32, 64, (0.02, 0.01, -0.03))
        t, face, bary = trace(o, d, v, f)
        dist, tc = line_distance(o, d, c)
        inner = (dist < 0.999 * r_in) & (tc > 0)
        assert inner.sum() > 20 and np.isfinite(t[inner]).all()
        t_out = tc[inner] - np.sqrt(r * r - dist[inner] ** 2)
        t_in = tc[inner] - np.sqrt(r_in * r_in - dist[inner] ** 2)
        assert (t[inner] >= t_out - 1e-6).all() and (t[inner] <= t_in + 1e-6).all()
        assert not np.isfinite(t[(dist > r * 1.0001) | (tc < 0)]).any()
        hit = (1 - bary.sum(1))[:, None] * vt[f[face, 0]] + bary[:, :1] * vt[f[face, 1]] + bary[:, 1:] * vt[f[face, 2]]
        ok = face >= 0
        np.testing.assert_allclose(hit[ok], (o + t[:, None] * d)[ok], atol=1e-12)


def test_tracer_rules():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float32)
    f = np.array([[3, 4, 5], [0, 1, 2], [0, 2, 1]], np.int32)  # z = 1, then z = 0 twice (both windings)
    o = np.array([[0.25, 0.25, -1.0], [0.25, 0.25, 0.5], [0.25, 0.25, 2.0], [2.0, 2.0, -1.0], [0.0, 0.25, -1.0]])
    d = np.array([[0, 0, 2.0], [0, 0, 2.0], [0, 0, 2.0], [0, 0, 1.0], [0, 0, 1.0]])
    t, face, bary = trace(o, d, v, f)
    assert np.allclose(t[:2], [0.5, 0.25]) and list(face[:4]) == [1, 0, -1, -1]  # t in units of d; ties: lowest index
    assert np.isinf(t[2]) and np.isinf(t[3]) and face[4] == 1 and bary[4, 0] == 0  # behind; outside; on an edge (inclusive)
    t2, face2, _ = trace(o, d, v, f, t_max=np.array([0.5, 1.0, 1.0, 1.0, 0.9]))
    assert list(face2) == [-1, 0, -1, -1, -1]  # t < t_max is exclusive
    assert trace(o, d, v, f[:0])[1].tolist() == [-1] * 5


# ----------------------------------------------------------------------------------------------- tests: shadow, hits
def test_shadow_ratio_properties():
    c, r = np.array([0.5, -0.1, 0.8]), 0.35
    v, f = icosphere(1, r, c)
    H, W = 8, 16
    dirs, omega = lspec.probe_dirs(H, W).astype(np.float32), lspec.probe_omega(H, W)
    probe = np.ones((H * W, 3))
    x = np.array([[0.5, -0.5, 0.8], [0.5, 0.6, 0.8], [np.nan, 0, 0], [30.0, -0.5, 0.8]], np.float32)
    n = np.tile(np.array([[0, 1, 0]], np.float32), (4, 1))
    ratio, share, pairs = shadow_ratio(x, n, probe, dirs, omega, v, f)
    assert 0 < ratio[0] < 0.9 and ratio[1] == 1.0 and ratio[2] == 1.0 and ratio[3] > 0.99 and pairs > 0
    assert (shadow_ratio(x, n, probe, dirs, omega, v, f[:0])[0] == 1.0).all()
    # uniform light: 1 - ratio under the sphere's centre is about the cosine-weighted solid angle / pi = (r / h)^2
    h = 0.4
    assert abs((1 - ratio[0]) - (r / h) ** 2) < 0.25


def test_hit_attributes_and_composite():
    v, f = icosphere(1, 0.35, (0.5, -0.1, 0.8))
    o, d = pinhole_rays(12, 16, 60.0, look_at((0.02, 0.01, -0.03), (0.5, -0.1, 0.8)))
    t, face, bary = trace(o, d, v, f)
    dep = np.full(len(t), 0.7)
    pos = np.array([[0.5, -0.1, 0.8], [0.2, 0.3, 0.4]])
    at = hit_attributes(o, d, t, face, bary, v, f, None, (0.2, 0.4, 0.6), dep, pos)
    m = at["mask"]
    assert m.any() and (m == ((face >= 0) & (t < dep))).all() and ((face >= 0) & ~m).any()
    c = np.array([0.5, -0.1, 0.8])
    radial = (at["points"][m] - c) / np.linalg.norm(at["points"][m] - c, axis=1, keepdims=True)
    assert ((at["normals"][m] * radial).sum(1) > 0.9).all()  # outward, towards the eye
    assert ((at["normals"][m] * at["viewdirs"][m]).sum(1) <= 0).all()
    np.testing.assert_allclose(at["weights"][m].sum(1), 1.0, atol=1e-12)
    assert (at["weights"][~m] == 0).all() and np.isnan(at["scene_points"][m]).all()
    np.testing.assert_allclose(at["scene_points"][~m], (o + 0.7 * d)[~m])
    # smooth normals of a sphere are radial
    vn = (v.astype(np.float64) - c) / 0.35
    at2 = hit_attributes(o, d, t, face, bary, v, f, vn, v.astype(np.float64), dep)
    assert ((at2["normals"][m] * radial).sum(1) > 0.995).all()
    np.testing.assert_allclose(at2["albedo"][m], at["points"][m], atol=1e-6)  # albedo = position blends to the hit point
    # a hit on a probe position takes that probe alone
    at3 = hit_attributes(o[m][:1], d[m][:1], t[m][:1], face[m][:1], bary[m][:1], v, f, None, (1, 1, 1), None,
                         np.stack([pos[1], at["points"][m][0]]))
    assert at3["weights"].tolist() == [[0.0, 1.0]]
    rgb, depth = composite(m, np.ones((len(t), 3)), t, np.full((len(t), 3), 0.5), dep, np.full(len(t), 0.5))
    assert (rgb[m] == 1).all() and (rgb[~m] == 0.25).all() and (depth[m] == t[m]).all() and (depth[~m] == 0.7).all()


# -------------------------------------------------------------------------------------------------------- tests: PLY
@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
def test_ply_round_trip(tmp_path, with_normals, with_colors):
    from pano_nerf_amd import geometry
    rng = np.random.default_rng(8)
    v, f = icosphere(1)
    n = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32) if with_normals else None
    c = (rng.integers(0, 256, v.shape) / 255.0).astype(np.float32) if with_colors else None
    path = str(tmp_path / "m.ply")
    geometry.write_ply(path, v, f, n, c)
    m = geometry.read_ply(path)
    assert isinstance(m, geometry.Mesh) and m.vertices.dtype == np.float32 and m.faces.dtype == np.int32
    assert np.array_equal(m.vertices, v) and np.array_equal(m.faces, f)
    assert (m.normals is None) == (n is None) and (m.colors is None) == (c is None)
    if n is not None:
        assert np.array_equal(m.normals, n)
    if c is not None:
        assert m.colors.dtype == np.float32 and np.abs(m.colors - c).max() < 1e-6
    # the ASCII form of the same elements
    head = open(path, "rb").read().split(b"end_header\n")[0].decode().replace("binary_little_endian", "ascii")
    lines = []
    for i in range(len(v)):
        row = [repr(float(x)) for x in v[i]] + ([repr(float(x)) for x in n[i]] if n is not None else [])
        row += [str(int(round(float(x) * 255))) for x in c[i]] if c is not None else []
        lines.append(" ".join(row))
    lines += ["3 %d %d %d" % tuple(t) for t in f]
    apath = str(tmp_path / "a.ply")
    open(apath, "w").write(head + "end_header\n" + "\n".join(lines) + "\n")
    a = geometry.read_ply(apath)
    assert np.array_equal(a.vertices, v) and np.array_equal(a.faces, f)
    if n is not None:
        assert np.array_equal(a.normals, n)
    if c is not None:
        assert np.abs(a.colors - c).max() < 1e-6


def test_ply_errors_name_what_they_found(tmp_path):
    from pano_nerf_amd import geometry
    v, f = icosphere(0)
    path = str(tmp_path / "m.ply")
    geometry.write_ply(path, v, f)
    raw = open(path, "rb").read()

    def variant(name, data):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        return p

    with pytest.raises(ValueError, match="binary_big_endian"):
        geometry.read_ply(variant("be.ply", raw.replace(b"binary_little_endian", b"binary_big_endian")))
    with pytest.raises(ValueError, match="double x"):
        geometry.read_ply(variant("dbl.ply", raw.replace(b"property float x", b"property double x")))
    with pytest.raises(ValueError, match="face properties"):
        geometry.read_ply(variant("lst.ply", raw.replace(b"list uchar int", b"list int int")))
    with pytest.raises(ValueError, match="not a PLY"):
        geometry.read_ply(variant("no.ply", b"solid\n"))
    with pytest.raises(ValueError, match="elements"):
        geometry.read_ply(variant("el.ply", raw.replace(b"element face", b"element edge")))
    head = raw.split(b"end_header\n")[0].replace(b"binary_little_endian", b"ascii")
    quad = head + b"end_header\n" + b"\n".join(b"%f %f %f" % tuple(x) for x in v) + b"\n" + b"4 0 1 2 3 \n" * len(f)
    with pytest.raises(ValueError, match="4 vertices"):
        geometry.read_ply(variant("quad.ply", quad))
    body = raw.split(b"end_header\n", 1)[1]
    nv = len(v) * 12
    with pytest.raises(ValueError, match="4 vertices"):
        geometry.read_ply(variant("quadb.ply", raw.split(b"end_header\n")[0] + b"end_header\n" + body[:nv] + b"\x04" + body[nv + 1:]))
    with pytest.raises(ValueError, match="ends early"):
        geometry.read_ply(variant("short.ply", raw[:-5]))


# ------------------------------------------------------------------------------------------- tests: argument checks
def test_argument_checks_that_need_no_device():
    import torch
    from pano_nerf_amd import objects
    z = torch.zeros(4, 3)
    faces = torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objects.trace_mesh(z, z, z, faces)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objects.shade(torch.zeros(1, 3, 4, 8), z, z, z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objects.shadow_ratio(z, z, torch.zeros(3, 4, 8), z, faces)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objects.VirtualObject(z, faces)
    with pytest.raises(ValueError, match=r"\[K, 3, H, W\]|\[P, 3, H, W\]"):
        objects.shade(torch.zeros(3, 4, 8), z, z, z)
    with pytest.raises(ValueError, match="VirtualObject"):
        objects.hit_attributes(None, z, z, z[:, 0], faces, z[:, :2])
    assert objects.MAX_PROBES == 8
