"""Baking on the GPU: the four kernels of pn_atlas.hip against the fp64 restatement of tests/_atlas_ref.py, baked maps read
back through the project's own sampler (VirtualObject.from_baked -> trace_mesh -> hit_attributes; sample_textures), the
model routes of bake_textures bit for bit against query_field and the renderer, write_obj -> VirtualObject.from_obj, and
argument errors.

Tolerances of the kernel tests (from the number formats, not from the kernels).  Both sides evaluate in fp64 on the same
fp32 inputs and round once to fp32, so an output differs from the rounded reference by at most one fp32 ulp of the value -
the two fp64 results differ by fp64 rounding noise, which can move a value across an fp32 rounding boundary - doubled as
the issue asks: 2 ulp32(value).  The fp64 noise itself matters only where an output is a difference of larger terms, and
is added per output as `noise`:
  uv, bary      quotients of small integers and half-integers, the same operations on both sides: no noise term
  points        w0 v0 + u v1 + v v2, five operations on terms of at most B = (|w0| + |u| + |v|) max|vertex| <= 4 max|vertex|
                (the gutter extrapolates by less than one leg): noise 8 * 2^-53 * 4 max|vertex| = 2^-48 max|vertex|
  normals_g     (e1 x e2) / A_w: each component of the cross product carries 3 * 2^-53 |e1| |e2|, A_w likewise, so the
                quotient carries 2^-50 K with K = |e1| |e2| / A_w, the face's conditioning, taken from the mesh
  var           A_w / (12 L^2): relative noise 2^-50 K
  normals_s     the blend divided by its norm: 2^-50 / |blend| (vertex normals are unit; |blend| >= 0.5 by construction)
  encoded       0.5 m + 0.5 with m a dot product of unit vectors, after two Gram-Schmidt steps.  Each step subtracts the part
                of T (of B) along N and divides by what is left, at least s = |N . n_g| of the vector (the sine of N's angle
                to the face's plane): the noise of T and B (2^-50 K, as for normals_g) grows by 1 / s per step:
                2^-48 K / s^2, with s taken per texel from the inputs (the random soups tilt N at will)
Bytes and face ids are exact.

Tolerances of the end-to-end tests are derived in their docstrings."""
import functools
import os

import numpy as np
import pytest
import torch

import _atlas_ref as ref
import _textures_ref as tref

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def T(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).to(dev())


def N(x):
    return x.detach().cpu().numpy()


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def within(got, want, noise, tag):
    """|got - fl32(want)| <= 2 ulp32(want) + noise, element by element; prints the worst error in ulp"""
    got = np.asarray(got, np.float64)
    w32 = ref.f32(want).astype(np.float64)
    assert got.shape == w32.shape, (tag, got.shape, w32.shape)
    err = np.abs(got - w32)
    bound = 2.0 * ulp32(w32) + noise
    worst = float((err / ulp32(w32)).max()) if err.size else 0.0
    print(f"{tag}: worst error {worst:.2f} ulp, {int((err > 0).sum())} of {err.size} values differ")
    assert np.all(err <= bound), (tag, worst, float(err.max()))


# ------------------------------------------------------------------------------------------- 1. the four kernels
SIZES = (6, 16, 37, 64)
FACES = (1, 2, 3, 7, 130)


def random_soup(F, seed):
    """F random faces over F + 3 vertices, with unit vertex normals scattered around one direction (so a blend of three is
    never short: |blend| >= 0.5) and unrelated to the faces.
    F >= 3: the last face has zero area; F >= 7: face 2 has an index outside [0, V), face 4 uses a NaN vertex."""
    rng = np.random.default_rng(seed)
    V = F + 3
    v = rng.uniform(-1.5, 1.5, (V, 3)).astype(np.float32)
    f = np.stack([rng.permutation(V - 1)[:3] for _ in range(F)]).astype(np.int32)  # vertex V - 1 is kept for the NaN
    n = rng.normal(size=(V, 3)) * 0.25 + np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    if F >= 3:
        f[F - 1] = (f[F - 1][0], f[F - 1][1], f[F - 1][0])
    if F >= 7:
        f[2, 1] = V + 5
        v[V - 1] = (0.25, np.nan, 1.0)
        f[4, 2] = V - 1
    return v, f, n


def conditioning(v, f, face):
    """K [S, S] = |e1| |e2| / A_w of each texel's face (1 where it has none, or no finite one)"""
    K = np.ones(len(f))
    p = v.astype(np.float64)
    for i, idx in enumerate(f):
        if np.all((idx >= 0) & (idx < len(v))) and np.isfinite(p[idx]).all():
            e1, e2 = p[idx[1]] - p[idx[0]], p[idx[2]] - p[idx[0]]
            A = np.linalg.norm(np.cross(e1, e2))
            if A > 0:
                K[i] = np.linalg.norm(e1) * np.linalg.norm(e2) / A
    return np.where(face >= 0, K[np.clip(face, 0, len(f) - 1)], 1.0)


@pytest.mark.parametrize("F", FACES)
@pytest.mark.parametrize("S", SIZES)
def test_kernels_match_the_restatement(S, F):
    from pano_nerf_amd import geometry
    v, f, n = random_soup(F, 100 * S + F)
    try:
        c = ref.cell_size(F, S)
    except ValueError:
        with pytest.raises(ValueError, match="too small"):  # no cell of 6 texels fits: refused, with the size that would do
            geometry.triangle_atlas(T(f, torch.int32), S)
        return
    at = geometry.triangle_atlas(T(f, torch.int32), S)
    assert (at.size, at.cell) == (S, c)
    assert at.uv.dtype == torch.float32 and tuple(at.uv.shape) == (3 * F, 2)
    assert at.face_uv.dtype == torch.int32 and np.array_equal(N(at.face_uv), np.arange(3 * F).reshape(F, 3))
    within(N(at.uv), ref.atlas_uv(F, S, c), 0.0, f"uv S={S} F={F}")
    assert bits_equal(at.uv, geometry.triangle_atlas(T(f, torch.int32), S).uv)
    vmax = float(np.nanmax(np.abs(v)))
    for normals in (None, n):
        tag = f"S={S} F={F} normals={'yes' if normals is not None else 'no'}"
        got = geometry.atlas_texels(T(v), T(f, torch.int32), at, None if normals is None else T(normals))
        want = ref.texels(S, c, v, f, normals)
        assert got["face"].dtype == torch.int32 and np.array_equal(N(got["face"]), want["face"]), tag
        K = conditioning(v, f, want["face"])
        within(N(got["bary"]), want["bary"], 0.0, tag + " bary")
        within(N(got["points"]), want["points"], 2.0 ** -48 * vmax, tag + " points")
        within(N(got["normals_g"]), want["normals_g"], (2.0 ** -50 * K)[..., None], tag + " normals_g")
        within(N(got["var"]), want["var"], 2.0 ** -50 * K * want["var"], tag + " var")
        within(N(got["normals_s"]), want["normals_s"], (2.0 ** -50 * (K if normals is None else np.full_like(K, 2.0)))[..., None],
               tag + " normals_s")
        for k in ("bary", "points", "normals_g", "normals_s", "var"):  # unowned texels: zeros, not merely small
            assert np.all(N(got[k])[want["face"] < 0] == 0), (tag, k)
        again = geometry.atlas_texels(T(v), T(f, torch.int32), at, None if normals is None else T(normals))
        for k in got:
            assert bits_equal(got[k], again[k]), (tag, k)
        # the encoder, on the kernel's own normals_s and UVs (fp32 inputs of both sides)
        rng = np.random.default_rng(S + F)
        Ns = N(got["normals_s"])
        world = Ns + 0.3 * rng.normal(size=Ns.shape)
        world /= np.maximum(np.linalg.norm(world, axis=2, keepdims=True), 1e-9)
        flat = world.reshape(-1, 3)
        flat[0::11] = -Ns.reshape(-1, 3)[0::11]   # faces away: (0.5, 0.5, 1)
        flat[1::13] = 0.0                         # no normal
        flat[2::17, 1] = np.nan
        world = world.astype(np.float32)
        enc = torch.empty(S, S, 3, device=dev())
        from pano_nerf_amd import _lib
        args = (S, c, F, len(v), T(v), T(f, torch.int32), at.uv, got["face"], got["normals_s"], T(world))
        call = lambda out: _lib.call("pn_atlas_encode_normals", *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args],
                                     out.data_ptr(), _lib.stream(dev()))
        call(enc)
        want_enc = ref.encode_normals(S, v, f, N(at.uv), want["face"], Ns, world)
        s_tilt = np.abs(np.einsum("ijc,ijc->ij", Ns.astype(np.float64), want["normals_g"]))
        amp = 1.0 / np.maximum(s_tilt, 1e-6) ** 2
        within(N(enc), want_enc, (2.0 ** -48 * K * amp)[..., None], tag + " encoded")
        fb = np.all(want_enc == (0.5, 0.5, 1.0), axis=2)
        assert np.all(N(enc)[fb] == np.array([0.5, 0.5, 1.0], np.float32)), tag
        assert fb[want["face"] < 0].all() and (not (want["face"] >= 0).any() or fb[want["face"] >= 0].any())
        enc2 = torch.empty_like(enc)
        call(enc2)
        assert bits_equal(enc, enc2), tag


@pytest.mark.parametrize("srgb", [None, False, True])
def test_quantiser_bytes_are_exact(srgb):
    from pano_nerf_amd import geometry
    t = tref.decode_table(bool(srgb))
    mid = ((t[:-1].astype(np.float64) + t[1:].astype(np.float64)) / 2).astype(np.float32)
    k = np.arange(255, dtype=np.float64)
    x = np.concatenate([t, mid, ((k + 0.5) / 255.0).astype(np.float32)])
    x = np.concatenate([x, np.nextafter(x, np.float32(-1)), np.nextafter(x, np.float32(2)),
                        np.array([-1.0, -0.0, 1.5, np.inf, -np.inf, np.nan, 1e-30, 0.5, 0.999999], np.float32),
                        np.random.default_rng(3).random(3 * 1001).astype(np.float32)]).astype(np.float32)
    x = x[:len(x) // 3 * 3].reshape(-1, 3)
    want = ref.quantize(x, None if srgb is None else t)
    got = geometry.quantize_image(T(x), srgb=bool(srgb), table=srgb is not None)
    assert got.dtype == torch.uint8 and tuple(got.shape) == x.shape
    np.testing.assert_array_equal(N(got), want)
    assert bits_equal(got, geometry.quantize_image(T(x), srgb=bool(srgb), table=srgb is not None))
    for C in (1, 2, 4):  # the channel count only shapes the rows
        xc = x.reshape(-1)[:x.size // C * C].reshape(-1, C)
        np.testing.assert_array_equal(N(geometry.quantize_image(T(xc), srgb=bool(srgb), table=srgb is not None)),
                                      ref.quantize(xc, None if srgb is None else t))
    assert tuple(geometry.quantize_image(torch.empty(0, 3, device=dev())).shape) == (0, 3)


# ------------------------------------------------------------------------------------------ 2. end to end: albedo
def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def split_octahedron():
    """every face of the octahedron split in three around a point close to its first edge: 8 slivers (a tenth of the
    face's height) and 16 large faces, still closed, every new face in its parent's plane"""
    v, f = octahedron()
    verts, faces = [p for p in v.astype(np.float64)], []
    for a, b, c in f:
        q = 0.45 * verts[a] + 0.45 * verts[b] + 0.10 * verts[c]
        verts.append(q)
        k = len(verts) - 1
        faces += [[a, b, k], [b, c, k], [c, a, k]]
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32)


A_MAT = np.array([[0.30, -0.20, 0.10], [-0.15, 0.25, 0.20], [0.10, 0.30, -0.25]])
B_VEC = np.array([0.5, 0.45, 0.55])


def affine_field(points, var, normals):
    p = points.double()
    return {"albedo": (p @ torch.as_tensor(A_MAT, device=p.device).T + torch.as_tensor(B_VEC, device=p.device)).float()}


def aimed_rays(v, f, seed):
    """rays from three radii out, aimed at random points of the faces, points 1e-4 (in barycentrics) from an edge, edge
    midpoints and vertices: (origins, directions, kind) with kind 0 interior, 1 near an edge, 2 on an edge, 3 at a vertex"""
    rng = np.random.default_rng(seed)
    p = v.astype(np.float64)
    tg, kind = [], []
    for i, (a, b, c) in enumerate(f):
        for _ in range(12):
            w = rng.dirichlet((1, 1, 1))
            tg.append(w[0] * p[a] + w[1] * p[b] + w[2] * p[c]); kind.append(0)
        for e in range(3):
            s = rng.uniform(0.05, 0.95)
            w = np.roll(np.array([s, 1 - s - 1e-4, 1e-4]), e)
            tg.append(w[0] * p[a] + w[1] * p[b] + w[2] * p[c]); kind.append(1)
            w = np.roll(np.array([0.5, 0.5, 0.0]), e)
            tg.append(w[0] * p[a] + w[1] * p[b] + w[2] * p[c]); kind.append(2)
        tg.append(p[a]); kind.append(3)
    tg = np.asarray(tg)
    o = 3.0 * tg / np.linalg.norm(tg, axis=1, keepdims=True)
    return o.astype(np.float32), (tg - o).astype(np.float32), np.asarray(kind)


@pytest.mark.parametrize("mesh", ["octahedron", "split"])
def test_affine_albedo_survives_bake_trace_and_sample(mesh):
    """An affine colour field a . p + b baked through the callable route and read back by the sampler at traced hits.

    Bilinear interpolation of an affine function over texels that lie on the triangle's plane (the gutter included: it
    continues that plane) is exact, so what is left is rounding.  With g = max_i sum_j |a_ij| (the colour's change per unit
    length, 0.75), M = g max|p| + max|b| (its magnitude, 1.3), e the longest edge, L the leg in texels, S = 64:
      the texel       its point is rounded once (<= 2^-24 max|p| per coordinate: g 2^-24), its colour once (2^-24 M)
      the sample      fp64 on fp32 UVs (3 corners, relative 2^-24, U <= 1) and fp32 barycentrics (2, relative 2^-24): the
                      sample moves by at most (S + 2 L) 2^-24 texels per axis, a texel is at most e / L long in the world:
                      2 g (e / L) (S + 2 L) 2^-24; the output is rounded once more (2^-24 M)
    which is the bound against a . p + b at the hit rebuilt from (face, bary) in fp64.  Against hit_attributes' own
    `points` = o + t d the tracer's fp32 t comes in: Moeller-Trumbore in fp32 on |o| = 3 carries some 16 roundings of
    2^-24 |o|, amplified by the face's conditioning K = |e1| |e2| / A_w and by 1 / cos of the incidence (>= 0.57 for rays
    along the radius of an octahedron): delta = 16 * 2^-24 * 3 K / 0.57, and the colour moves by g delta.
    Without the gutter rule the hits on edges read texels of other faces, or empty ones: errors of 0.01 .. 0.5."""
    from pano_nerf_amd import geometry, objects
    v, f = octahedron() if mesh == "octahedron" else split_octahedron()
    S = 64
    m = geometry.Mesh(T(v), T(f, torch.int32), None, None)
    baked = geometry.bake_textures(affine_field, m, size=S, maps=("albedo", "coverage"))
    c = ref.cell_size(len(f), S)
    L = c - 4
    assert tuple(baked.maps["albedo"].shape) == (S, S, 3) and tuple(baked.maps["coverage"].shape) == (S, S, 1)
    own = ref.owners(S, c, len(f))[0] >= 0
    assert np.array_equal(N(baked.maps["coverage"])[..., 0] == 1, own) and np.all(N(baked.maps["albedo"])[~own] == 0)
    obj = objects.VirtualObject.from_baked(baked)
    o, d, kind = aimed_rays(v, f, 11)
    t, face, bary = objects.trace_mesh(T(o), T(d), obj.vertices, obj.faces)
    att = objects.hit_attributes(obj, T(o), T(d), t, face, bary, radii=None)
    mask = N(att["mask"])
    assert mask.mean() >= 0.97 and mask[kind == 0].all() and mask[kind >= 2].mean() >= 0.9, (mask.mean(), mask[kind >= 2].mean())
    assert len(o) >= 150
    p = v.astype(np.float64)
    fa, bc = N(face)[mask], N(bary)[mask].astype(np.float64)
    tri = p[f[fa]]
    rebuilt = (1 - bc[:, :1] - bc[:, 1:]) * tri[:, 0] + bc[:, :1] * tri[:, 1] + bc[:, 1:] * tri[:, 2]
    got = N(att["albedo"])[mask].astype(np.float64)
    g = float(np.abs(A_MAT).sum(1).max())
    M = g * 1.0 + float(B_VEC.max())
    e1, e2 = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
    e3 = p[f[:, 2]] - p[f[:, 1]]
    emax = float(max(np.linalg.norm(e1, axis=1).max(), np.linalg.norm(e2, axis=1).max(), np.linalg.norm(e3, axis=1).max()))
    K = float((np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) / np.linalg.norm(np.cross(e1, e2), axis=1)).max())
    u = 2.0 ** -24
    tol_bary = g * u + M * u + 2 * g * (emax / L) * (S + 2 * L) * u + M * u
    tol_points = tol_bary + g * 16 * u * 3.0 * K / 0.57
    err_b = np.abs(got - (rebuilt @ A_MAT.T + B_VEC)).max(1)
    err_p = np.abs(got - (N(att["points"])[mask].astype(np.float64) @ A_MAT.T + B_VEC)).max(1)
    for k in range(4):
        sel = kind[mask] == k
        print(f"{mesh}: kind {k}: {int(sel.sum())} hits, max error {err_b[sel].max():.3g} at the rebuilt hit (bound "
              f"{tol_bary:.3g}), {err_p[sel].max():.3g} at points (bound {tol_points:.3g})")
    assert np.all(err_b <= tol_bary), (float(err_b.max()), tol_bary)
    assert np.all(err_p <= tol_points), (float(err_p.max()), tol_points)


# ----------------------------------------------------------------------------------------- 3. end to end: normals
@functools.lru_cache(maxsize=None)
def icosphere():
    """the icosahedron subdivided once (42 vertices, 80 faces) on the unit sphere around CENTRE, outward winding"""
    ph = (1 + 5 ** 0.5) / 2
    v = [(-1, ph, 0), (1, ph, 0), (-1, -ph, 0), (1, -ph, 0), (0, -1, ph), (0, 1, ph), (0, -1, -ph), (0, 1, -ph),
         (ph, 0, -1), (ph, 0, 1), (-ph, 0, -1), (-ph, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    mid, out = {}, []

    def midpoint(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            q = v[a] + v[b]
            v.append(q / np.linalg.norm(q))
            mid[key] = len(v) - 1
        return mid[key]

    for a, b, c in f:
        ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    unit = np.asarray(v)
    return (unit + CENTRE).astype(np.float32), np.asarray(out, np.int32), unit.astype(np.float32)


CENTRE = np.array([0.1, -0.2, 0.3])
# the field's centre is NOT the sphere's: around the sphere's own centre normalize(p - centre) of a point of a face is the
# normalised blend of the vertex normals itself, m = (0, 0, 1) everywhere, and the tangent frame would never be used
FIELD_CENTRE = CENTRE + np.array([0.25, -0.15, 0.2])


def sphere_normal_field(points, var, normals):
    q = points.double() - torch.as_tensor(FIELD_CENTRE, device=points.device)
    return {"normal": (q / q.norm(dim=1, keepdim=True)).float()}


def centre_hits(tex):
    """the owned texels whose centre lies inside their triangle: flat indices, faces, barycentrics"""
    face, bary = N(tex["face"]).reshape(-1), N(tex["bary"]).reshape(-1, 2)
    sel = np.nonzero((face >= 0) & (bary[:, 0] >= 0) & (bary[:, 1] >= 0) & (bary.sum(1) <= 1))[0]
    return sel, face[sel], bary[sel]


def test_baked_normals_decode_to_the_field():
    """normalize(p - centre) (centre 0.35 off the sphere's own, so that the normal tilts up to 20 degrees against the
    vertex normals) baked on an icosphere with vertex normals, then sampled at hits placed at the centres of owned
    in-triangle texels with directions = -normals_s: the sampler returns the baked normal.

    The stored texel is 0.5 m + 0.5, rounded once per component (<= 2^-25 each, values in [0, 1]); the sampler forms
    m = 2 s - 1 (2^-24 per component, sqrt(3) 2^-24 on the vector), rebuilds n in the same frame from the same fp32 inputs
    in fp64, and rounds once (2^-24): (sqrt(3) + 1) 2^-24, doubled for values that cross a rounding boundary.
    The hit is not exactly on the texel's centre: its barycentrics and the corner UVs are fp32 (relative 2^-24), which
    moves the sample by at most w = (S + 2 L) 2^-24 texels per axis and mixes in the neighbouring texels with that weight.
    Neighbouring texels differ by at most D per component: over one texel (<= e / L of world length, e the longest edge)
    the baked normal turns by <= (e / L) / r (r the smallest |p - centre| over the texels, >= 0.5), the frame (N, T', B')
    by the turn of the blended vertex normals, <= (e / L) / 0.9 each (the blend of unit normals of one face is never
    shorter than 0.9), so m moves by <= (1 / r + 2 / 0.9) e / L and the texel by half of it: D.  Two axes, m = 2 s - 1,
    three components: sqrt(3) * 2 * 2 w D.
    A map holding (0.5, 0.5, 1) everywhere decodes to N itself."""
    from pano_nerf_amd import geometry, objects
    v, f, vn = icosphere()
    S = 64
    m = geometry.Mesh(T(v), T(f, torch.int32), T(vn), None)
    baked = geometry.bake_textures(sphere_normal_field, m, size=S, maps=("normal", "normal_world"))
    c = ref.cell_size(len(f), S)
    L = c - 4
    at = geometry.triangle_atlas(m.faces, S)
    assert bits_equal(at.uv, baked.uv) and at.cell == c
    tex = geometry.atlas_texels(m.vertices, m.faces, at, m.normals)
    sel, face, bary = centre_hits(tex)
    assert len(sel) >= len(f), len(sel)
    # the baked maps are what the pieces give
    want_world = np.zeros((S * S, 3), np.float32)
    own = N(tex["face"]).reshape(-1) >= 0
    q = N(tex["points"]).reshape(-1, 3)[own].astype(np.float64) - FIELD_CENTRE
    want_world[own] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    assert np.abs(N(baked.maps["normal_world"]).reshape(-1, 3) - want_world).max() <= 2.0 ** -23
    enc_ref = ref.encode_normals(S, v, f, N(at.uv), N(tex["face"]), N(tex["normals_s"]), N(baked.maps["normal_world"]))
    within(N(baked.maps["normal"]), enc_ref, 2.0 ** -40, "baked normal map")
    obj = objects.VirtualObject.from_baked(baked)
    Ns = tex["normals_s"].reshape(-1, 3)[T(sel, torch.int64)]
    R = len(sel)
    out = objects.sample_textures(obj, torch.ones(R, dtype=torch.bool, device=dev()), T(face, torch.int32), T(bary), -Ns,
                                  torch.ones(R, device=dev()), Ns, radii=None)
    got = N(out["normals"]).astype(np.float64)
    want = N(baked.maps["normal_world"]).reshape(-1, 3)[sel].astype(np.float64)
    p = v.astype(np.float64)
    emax = max(float(np.linalg.norm(p[f[:, a]] - p[f[:, b]], axis=1).max()) for a, b in ((0, 1), (1, 2), (2, 0)))
    r = float(np.linalg.norm(q, axis=1).min())
    assert r >= 0.5, r
    u = 2.0 ** -24
    w, D = (S + 2 * L) * u, 0.5 * (1.0 / r + 2.0 / 0.9) * emax / L
    tol = 2 * (3 ** 0.5 + 1) * u + 3 ** 0.5 * 2 * 2 * w * D
    err = np.abs(got - want).max()
    print(f"decoded normals: {R} hits, max error {err:.3g} (bound {tol:.3g}; rounding alone {2 * (3 ** 0.5 + 1) * u:.3g})")
    assert err <= tol, (err, tol)
    assert np.all(N(out["lod"]) == 0)
    tilt = np.einsum("rc,rc->r", want, N(Ns).astype(np.float64))
    assert tilt.min() > 0.5 and tilt.min() < 0.97, tilt.min()  # the frame is used, and no texel fell back
    assert not np.any(np.all(N(baked.maps["normal"]).reshape(-1, 3)[sel] == np.float32([0.5, 0.5, 1.0]), axis=1))
    # the fall-back texel: N, bit for bit
    flat = torch.tensor([0.5, 0.5, 1.0], device=dev()).expand(S, S, 3).contiguous()
    obj_flat = objects.VirtualObject(m.vertices, m.faces, m.normals, uv=baked.uv, face_uv=baked.face_uv,
                                     normal_map=objects.Texture(flat))
    out_flat = objects.sample_textures(obj_flat, torch.ones(R, dtype=torch.bool, device=dev()), T(face, torch.int32),
                                       T(bary), -Ns, torch.ones(R, device=dev()), Ns, radii=None)
    a, b = N(out_flat["normals"]), N(Ns)
    diff = a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)
    print(f"fall-back texel: {int((diff != 0).any(1).sum())} of {R} rows differ from N, by at most {int(np.abs(diff).max())} ulp")
    assert bits_equal(out_flat["normals"], Ns)


# ------------------------------------------------------------------------------------------- 4. the model routes
def make_model(cls):
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    nc = 5 if cls == "pano" else 1
    extra = dict(mlp_num_density_channels=5, num_env_samples=10) if cls == "pano" else {}
    model = (pn.PanoMipNeRF if cls == "pano" else pn.MipNeRF)(num_samples=16, rgb_activation="softplus", **extra)
    model.mlp.load_state_dict(orc.init_params(4, nc))
    return model.to(dev())


def octa_mesh():
    from pano_nerf_amd import geometry
    v, f = octahedron()
    vn = v / np.linalg.norm(v, axis=1, keepdims=True)
    return geometry.Mesh(T(v * 0.7), T(f, torch.int32), T(vn), None)


def test_point_method_is_query_field_bit_for_bit():
    from pano_nerf_amd import geometry
    model, m, S = make_model("pano"), octa_mesh(), 32
    baked = geometry.bake_textures(model, m, size=S, maps=("albedo", "radiance", "normal_world", "normal", "coverage"))
    tex = geometry.atlas_texels(m.vertices, m.faces, geometry.triangle_atlas(m.faces, S), m.normals)
    own = tex["face"].reshape(-1) >= 0
    assert int(own.sum()) == 4 * 16 * 16 and bits_equal(baked.maps["coverage"].reshape(-1), own.float())
    pts, var = tex["points"].reshape(-1, 3)[own], tex["var"].reshape(-1)[own]
    var3 = var[:, None].expand(-1, 3).contiguous()
    q = geometry.query_field(model, pts, var3, outputs=("albedo", "normal"))
    rgb = geometry.query_field(model, pts, var3, viewdirs=-tex["normals_s"].reshape(-1, 3)[own], outputs=("rgb",))["rgb"]
    for name, want in (("albedo", q["albedo"]), ("normal_world", q["normal"]), ("radiance", rgb)):
        got = baked.maps[name].reshape(-1, 3)
        assert bits_equal(got[own], want), name
        assert bool((got[~own] == 0).all()), name
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0, name
    # chunked evaluation, and a MipNeRF's radiance and normals
    again = geometry.bake_textures(model, m, size=S, maps=("albedo",), chunk_rows=300)
    assert bits_equal(again.maps["albedo"], baked.maps["albedo"])
    mip = make_model("mip")
    b2 = geometry.bake_textures(mip, m, size=S, maps=("radiance", "normal"))
    assert bool(torch.isfinite(b2.maps["normal"]).all()) and float(b2.maps["radiance"].abs().max()) > 0
    with pytest.raises(ValueError, match="albedo needs a 5-channel density head"):
        geometry.bake_textures(mip, m, size=S, maps=("albedo",))
    with pytest.raises(ValueError, match="albedo needs a 5-channel density head"):
        geometry.bake_textures(mip, m, size=S, maps=("albedo",), method="ray")


def test_ray_method_is_the_renderer_bit_for_bit():
    import pano_nerf_amd as pn
    from pano_nerf_amd import geometry
    model, m, S = make_model("pano"), octa_mesh(), 32
    env = pn.generate_lit_rays(10, 3.0)
    tex = geometry.atlas_texels(m.vertices, m.faces, geometry.triangle_atlas(m.faces, S), m.normals)
    rays, idx = geometry.atlas_rays(tex)
    own = tex["face"].reshape(-1) >= 0
    assert torch.equal(idx, torch.nonzero(own).reshape(-1))
    # the rays: from `offset` above the face to `offset` below it, a cone one texel wide at the face
    var = tex["var"].reshape(-1)[own]
    offset = float(4.0 * torch.sqrt(12.0 * var.median()))
    ng = tex["normals_g"].reshape(-1, 3)[own]
    assert bits_equal(rays.origins, tex["points"].reshape(-1, 3)[own] + offset * ng) and bits_equal(rays.directions, -ng)
    assert bits_equal(rays.viewdirs, -ng) and bool((rays.near == 0).all()) and bits_equal(rays.far, torch.full_like(rays.far, 2 * offset))
    width = 2.0 * N(rays.radii)[:, 0].astype(np.float64) * offset   # the cone's width where it meets the face
    np.testing.assert_allclose(width, np.sqrt(12.0 * N(var).astype(np.float64)), rtol=1e-6)
    with torch.no_grad():
        _, fine = model(rays=rays, env_rays=env, randomized=False, white_bkgd=False, enable_surf=True, use_ort_loss=False)
    baked = geometry.bake_textures(model, m, size=S, maps=("albedo", "radiance", "normal_world"), method="ray", env_rays=env)
    for name, want in (("radiance", fine[0]), ("normal_world", fine[3]), ("albedo", fine[4])):
        got = baked.maps[name].reshape(-1, 3)
        assert bits_equal(got[own], want.detach()), name
        assert bool((got[~own] == 0).all()) and float(got.nan_to_num().abs().max()) > 0, name
    with torch.no_grad():  # without the surface pass: the same rgb and normals
        _, fine2 = model(rays=rays, env_rays=None, randomized=False, white_bkgd=False, enable_surf=False, use_ort_loss=False)
    b2 = geometry.bake_textures(model, m, size=S, maps=("radiance", "normal_world"), method="ray", offset=offset)
    assert bits_equal(b2.maps["radiance"].reshape(-1, 3)[own], fine2[0].detach())
    assert bits_equal(b2.maps["normal_world"].reshape(-1, 3)[own], fine2[3].detach())
    with pytest.raises(ValueError, match="env_rays"):
        geometry.bake_textures(model, m, size=S, maps=("albedo",), method="ray")
    with pytest.raises(ValueError, match="method"):
        geometry.bake_textures(model, m, size=S, method="splat")


# ------------------------------------------------------------------------------------------ 5. files and errors
def colour_and_normal_field(points, var, normals):
    out = affine_field(points, var, normals)
    out.update(sphere_normal_field(points + torch.as_tensor(CENTRE, device=points.device).float(), var, normals))  # an octahedron around 0
    out["radiance"] = out["albedo"] * 7.0
    return out


@pytest.mark.parametrize("fmt", ["png", "exr"])
def test_write_obj_is_read_by_from_obj(tmp_path, fmt):
    from pano_nerf_amd import geometry, objects
    m, S = octa_mesh(), 32
    baked = geometry.bake_textures(colour_and_normal_field, m, size=S, maps=("albedo", "normal", "radiance"))
    path = str(tmp_path / "octa.obj")
    files = geometry.write_obj(path, baked, image_format=fmt)
    assert sorted(os.path.basename(p) for p in files.values()) == [f"octa_albedo.{fmt}", f"octa_normal.{fmt}", "octa_radiance.exr"]
    obj = objects.VirtualObject.from_obj(path, device=dev())
    assert bits_equal(obj.vertices, baked.vertices) and bits_equal(obj.faces, baked.faces) and bits_equal(obj.normals, baked.normals)
    assert bits_equal(obj.uv, baked.uv) and bits_equal(obj.face_uv, baked.face_uv) and obj.flip_v
    assert (obj.albedo_map.H, obj.albedo_map.W, obj.normal_map.H, obj.normal_map.W) == (S, S, S, S)
    if fmt == "png":
        for tex, name, srgb in ((obj.albedo_map, "albedo", True), (obj.normal_map, "normal", False)):
            code = geometry.quantize_image(baked.maps[name], srgb=srgb)
            np.testing.assert_array_equal(N(code), ref.quantize(N(baked.maps[name]), tref.decode_table(srgb)))
            table = torch.from_numpy(tref.decode_table(srgb)).to(dev())
            assert bits_equal(tex.level(0)[..., :3].contiguous(), table[code.long()]), name
            # the nearest code: decoding it lands within half a table step of the clamped value
            step = float(np.diff(tref.decode_table(srgb).astype(np.float64)).max())
            assert float((tex.level(0)[..., :3] - baked.maps[name].clamp(0, 1)).abs().max()) <= step / 2 + 2.0 ** -24, name
    else:
        assert bits_equal(obj.albedo_map.level(0)[..., :3].contiguous(), baked.maps["albedo"])
        assert bits_equal(obj.normal_map.level(0)[..., :3].contiguous(), baked.maps["normal"])
    from pano_nerf_amd import io_exr
    assert np.array_equal(io_exr.read_exr(files["radiance"]).view(np.uint32), N(baked.maps["radiance"]).view(np.uint32))


def test_export_scene_writes_a_loadable_asset(tmp_path):
    """extract_mesh -> bake_textures -> write_obj in one call, on a random model: the files exist, load, and hold the maps"""
    from pano_nerf_amd import geometry, objects
    model = make_model("pano")
    bounds, res = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), 8  # at most 7^3 cubes x 12 faces: fits 512 x 512 at any level
    sigma = geometry.density_grid(model, bounds, res)
    level = float(sigma.median())
    path = str(tmp_path / "scene.obj")
    baked = geometry.export_scene(model, bounds, res, level, path, size=512, maps=("albedo", "normal"))
    F = int(baked.faces.shape[0])
    assert F > 0 and tuple(baked.uv.shape) == (3 * F, 2) and tuple(baked.maps["albedo"].shape) == (512, 512, 3)
    obj = objects.VirtualObject.from_obj(path, device=dev())
    assert bits_equal(obj.vertices, baked.vertices) and bits_equal(obj.faces, baked.faces) and bits_equal(obj.uv, baked.uv)
    code = geometry.quantize_image(baked.maps["albedo"], srgb=True)
    table = torch.from_numpy(tref.decode_table(True)).to(dev())
    assert bits_equal(obj.albedo_map.level(0)[..., :3].contiguous(), table[code.long()])


def test_argument_errors():
    from pano_nerf_amd import geometry, _lib
    v, f = octahedron()
    with pytest.raises(RuntimeError, match="HIP device only"):
        geometry.triangle_atlas(torch.from_numpy(f), 32)
    at = geometry.triangle_atlas(T(f, torch.int32), 32)
    with pytest.raises(RuntimeError, match="HIP device only"):
        geometry.atlas_texels(torch.from_numpy(v), T(f, torch.int32), at)
    with pytest.raises(RuntimeError, match="HIP device only"):
        geometry.bake_textures(affine_field, geometry.Mesh(torch.from_numpy(v), torch.from_numpy(f), None, None), size=32)
    with pytest.raises(RuntimeError, match="HIP device only"):
        geometry.quantize_image(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="size >= 12 would do"):  # 8 faces: 2 x 2 cells of 6 texels
        geometry.triangle_atlas(T(f, torch.int32), 11)
    with pytest.raises(ValueError, match="too small"):
        geometry.bake_textures(affine_field, geometry.Mesh(T(v), T(f, torch.int32), None, None), size=8)
    with pytest.raises(ValueError, match="cell must be"):
        geometry.triangle_atlas(T(f, torch.int32), 32, cell=17)
    assert geometry.triangle_atlas(T(f, torch.int32), 32, cell=7).cell == 7
    with pytest.raises(ValueError, match="unknown maps"):
        geometry.bake_textures(affine_field, geometry.Mesh(T(v), T(f, torch.int32), None, None), size=32, maps=("gloss",))
    with pytest.raises(ValueError, match="need"):
        geometry.bake_textures(affine_field, geometry.Mesh(T(v), T(f, torch.int32), None, None), size=32, maps=("normal",))
    # the entry points refuse what the layout cannot hold, and NULL outputs
    lib = _lib.load()
    uv = torch.empty(24, 2, device=dev())
    bad_shape, null = lib.pn_atlas_uv(8, 11, 5, uv.data_ptr(), None), lib.pn_atlas_uv(8, 32, 16, None, None)
    assert b"shape" in lib.pn_strerror(bad_shape).lower() and bad_shape != 0 and null != 0 and null != bad_shape
    assert lib.pn_atlas_uv(9, 32, 16, uv.data_ptr(), None) == bad_shape  # 9 faces in 2 x 2 cells
    assert lib.pn_atlas_uv(0, 32, 16, None, None) == 0 and lib.pn_atlas_quantize(0, 3, None, None, None, None) == 0
    assert lib.pn_atlas_quantize(4, 5, uv.data_ptr(), None, uv.data_ptr(), None) == bad_shape
