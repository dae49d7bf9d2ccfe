"""fp64 numpy restatement of the lighting contract (include/panonerf_hip.h, pano_nerf_amd.lighting): probe directions
and solid angles, the real SH basis (l <= 2), SH projection, the exact cosine-weighted quadrature, Ramamoorthi-Hanrahan
irradiance and trilinear sampling of an SH volume.  Checked here against the reference's own outputs
(tests/golden/lighting_ref.npz) and analytic cases; test_gpu_lighting.py checks the kernels against it."""
import math

import numpy as np
import pytest

from conftest import load_golden

C0, C1, C2, C3, C4 = 0.28209479177387814, 0.48860251190291992, 1.0925484305920792, 0.31539156525252005, 0.54627421529603959
A_HAT = np.array([math.pi] + [2 * math.pi / 3] * 3 + [math.pi / 4] * 5)


def probe_dirs(H, W):
    """[H W, 3] unit directions of the probe pixels (sample_dir_by_pano, fp64)."""
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    theta = -(j + 0.5) / W * 2 * np.pi
    phi = (i + 0.5) / H * np.pi
    d = np.stack([np.sin(phi) * np.sin(theta), np.cos(phi), np.sin(phi) * np.cos(theta)], -1)
    return d.reshape(-1, 3)


def probe_omega(H, W):
    """[H W] pixel solid angles sin((i + 1/2) pi / H) (2 pi / W) (pi / H) (fp64)."""
    y = (np.arange(H) + 0.5) / H
    return (np.sin(y * np.pi)[:, None] * (2 * np.pi / W) * (np.pi / H) * np.ones((1, W))).reshape(-1)


def sh_basis(d):
    """[..., 9] real SH at directions d [..., 3] in the order (0,0) (1,-1) (1,0) (1,1) (2,-2) (2,-1) (2,0) (2,1) (2,2)."""
    d = np.asarray(d, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, C0), C1 * y, C1 * z, C1 * x, C2 * x * y, C2 * y * z, C3 * (3 * z * z - 1),
                     C2 * x * z, C4 * (x * x - y * y)], -1)


def as_pixels(probes):
    """[P, 3, H, W] -> [P, H W, 3] fp64."""
    p = np.asarray(probes, dtype=np.float64)
    return p.reshape(p.shape[0], 3, -1).transpose(0, 2, 1)


def sh_project(L, dirs, omega):
    """L [P, HW, 3] -> [P, 9, 3]: sum_pix L(pix) Y(dir_pix) omega_pix."""
    Y = sh_basis(dirs) * np.asarray(omega, np.float64)[:, None]  # [HW, 9]
    return np.einsum("pnc,nk->pkc", np.asarray(L, np.float64), Y)


def irradiance_exact(L, normals, dirs, omega):
    """L [P, HW, 3], normals [P or 1, K, 3] -> [P, K, 3]: sum_pix L(pix) max(0, n . dir_pix) omega_pix."""
    n = np.asarray(normals, np.float64)
    cos = np.einsum("qkc,nc->qkn", n, np.asarray(dirs, np.float64))
    cos = np.where(cos < 0, 0.0, cos)  # relu: NaN stays NaN
    w = cos * np.asarray(omega, np.float64)[None, None]
    return np.einsum("qkn,pnc->pkc", w, np.asarray(L, np.float64)) if n.shape[0] == 1 else \
        np.einsum("pkn,pnc->pkc", w, np.asarray(L, np.float64))


def sh_irradiance(sh, normals):
    """sh [P, 9, 3], normals [P or 1, K, 3] -> [P, K, 3]: sum A_l L_lm Y_lm(n)."""
    Y = sh_basis(normals) * A_HAT  # [Q, K, 9]
    sh = np.asarray(sh, np.float64)
    return np.einsum("qkj,pjc->pkc", Y, sh) if Y.shape[0] == 1 else np.einsum("pkj,pjc->pkc", Y, sh)


def trilinear(grid, lo, step, points):
    """grid [nx, ny, nz, ...] of vertex values at lo + (i, j, k) step; points [M, 3] clamped to the box -> [M, ...]."""
    g = np.asarray(grid, np.float64)
    res = np.array(g.shape[:3])
    u = (np.asarray(points, np.float64) - np.asarray(lo, np.float64)) / np.asarray(step, np.float64)
    u = np.clip(u, 0, res - 1)
    i0 = np.minimum(np.floor(u).astype(int), res - 2)
    t = u - i0
    out = 0
    for c in range(8):
        b = np.array([c >> 2, (c >> 1) & 1, c & 1])
        w = np.prod(np.where(b, t, 1 - t), axis=1)
        idx = i0 + b
        out = out + w.reshape((-1,) + (1,) * (g.ndim - 3)) * g[idx[:, 0], idx[:, 1], idx[:, 2]]
    return out


def volume_irradiance(grid, lo, step, points, normals):
    """SH volume grid [nx, ny, nz, 9, 3] -> [M, 3] at points [M, 3] for normals [M, 3]."""
    L = trilinear(grid, lo, step, points)  # [M, 9, 3]
    Y = sh_basis(normals) * A_HAT
    return np.einsum("mj,mjc->mc", Y, L)


def random_unit(rng, *shape):
    n = rng.standard_normal(shape + (3,))
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("size", ["8x16", "16x32"])
def test_conventions_match_the_reference(size):
    g = load_golden("lighting_ref")
    H, W = (int(s) for s in size.split("x"))
    np.testing.assert_allclose(probe_dirs(H, W), g[size + "/dirs"], rtol=2e-6, atol=2e-7)
    assert np.array_equal(probe_omega(H, W).astype(np.float32), g[size + "/omega"])


@pytest.mark.parametrize("size", ["8x16", "16x32"])
def test_quadrature_is_the_reference_shading(size):
    g = load_golden("lighting_ref")
    env, n = g[size + "/env"], g[size + "/normal"]
    got = irradiance_exact(env, n[:, None], g[size + "/dirs"], g[size + "/omega"])[:, 0]
    np.testing.assert_allclose(got, g[size + "/shading"], rtol=2e-6, atol=1e-6 * np.abs(got).max())


def test_solid_angles_sum_to_the_documented_error():
    for H in (8, 32, 128):
        err = probe_omega(H, 2 * H).sum() / (4 * np.pi) - 1
        assert abs(err - (np.pi / H) ** 2 / 24) < 0.02 * (np.pi / H) ** 2 / 24, (H, err)


def test_constant_radiance_gives_pi():
    rng = np.random.default_rng(0)
    H, W = 64, 128
    dirs, om = probe_dirs(H, W), probe_omega(H, W)
    L = np.broadcast_to(np.array([1.0, 2.0, 0.5]), (1, H * W, 3))
    n = random_unit(rng, 1, 16)
    E = irradiance_exact(L, n, dirs, om)[0]
    np.testing.assert_allclose(E, np.pi * np.array([1.0, 2.0, 0.5])[None].repeat(16, 0), rtol=2e-3)
    # along the pole axis the clamp falls on a pixel-row boundary: the midpoint rule's error on sin(phi) cos(phi),
    # (pi / H)^2 / 6 relative
    E_up = irradiance_exact(L, np.array([[[0.0, 1.0, 0.0]]]), dirs, om)[0, 0]
    assert abs(E_up[0] / np.pi - 1 - (np.pi / H) ** 2 / 6) < 0.05 * (np.pi / H) ** 2 / 6
    # SH route: E = A_0 L_00 Y_00 = pi for a constant
    sh = sh_project(L, dirs, om)
    np.testing.assert_allclose(sh_irradiance(sh, n)[0], E, rtol=2e-3)


def test_basis_functions_project_to_unit_vectors():
    H, W = 64, 128
    dirs, om = probe_dirs(H, W), probe_omega(H, W)
    Y = sh_basis(dirs)
    for k in range(9):
        L = np.repeat(Y[None, :, k:k + 1], 3, axis=2)
        sh = sh_project(L, dirs, om)[0]
        want = np.zeros((9, 3))
        want[k] = 1.0
        np.testing.assert_allclose(sh, want, atol=2e-3)


def test_band_limited_radiance_sh_equals_quadrature():
    rng = np.random.default_rng(1)
    H, W = 64, 128
    dirs, om = probe_dirs(H, W), probe_omega(H, W)
    coef = rng.standard_normal((2, 9, 3))
    coef[:, 0] = 4.0  # keep the radiance positive-ish; positivity is not needed for the identity
    L = np.einsum("nk,pkc->pnc", sh_basis(dirs), coef)
    n = random_unit(rng, 2, 32)
    exact = irradiance_exact(L, n, dirs, om)
    via_sh = sh_irradiance(sh_project(L, dirs, om), n)
    analytic = sh_irradiance(coef, n)
    scale = np.abs(analytic).max()
    assert np.abs(exact - analytic).max() < 3e-3 * scale
    assert np.abs(via_sh - analytic).max() < 3e-3 * scale


def test_per_probe_and_shared_normals_agree():
    rng = np.random.default_rng(2)
    H, W = 8, 16
    dirs, om = probe_dirs(H, W), probe_omega(H, W)
    L = rng.random((3, H * W, 3))
    n = random_unit(rng, 1, 5)
    a = irradiance_exact(L, n, dirs, om)
    b = irradiance_exact(L, np.repeat(n, 3, axis=0), dirs, om)
    np.testing.assert_allclose(a, b, rtol=1e-14)
    Ln = L.copy()
    Ln[1, 7, 0] = np.nan
    e = irradiance_exact(Ln, n, dirs, om)
    assert np.all(np.isnan(e[1, :, 0])) and np.all(np.isfinite(e[0])) and np.all(np.isfinite(e[1, :, 1:]))


def test_trilinear_vertices_centres_and_clamping():
    rng = np.random.default_rng(3)
    res, lo, step = (4, 3, 5), np.array([-1.0, 0.5, 2.0]), np.array([0.5, 0.25, -0.75])
    g = rng.standard_normal(res + (9, 3))
    i, j, k = np.meshgrid(*[np.arange(r) for r in res], indexing="ij")
    verts = lo + np.stack([i, j, k], -1).reshape(-1, 3) * step
    np.testing.assert_allclose(trilinear(g, lo, step, verts), g.reshape(-1, 9, 3), atol=1e-12)
    centre = lo + (np.array([1, 0, 2]) + 0.5) * step
    corners = [g[1 + a, 0 + b, 2 + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    np.testing.assert_allclose(trilinear(g, lo, step, centre[None])[0], np.mean(corners, 0), atol=1e-12)
    outside = lo + np.array([[-3.0, -1.0, 10.0]]) * step  # below x and y, above z: clamps to vertex (0, 0, nz - 1)
    np.testing.assert_allclose(trilinear(g, lo, step, outside)[0], g[0, 0, res[2] - 1], atol=1e-12)
    n = random_unit(rng, 4)
    e = volume_irradiance(g, lo, step, verts[:4], n)
    want = np.stack([sh_irradiance(g.reshape(-1, 9, 3)[m:m + 1], n[None, m:m + 1])[0, 0] for m in range(4)])
    np.testing.assert_allclose(e, want, atol=1e-12)
