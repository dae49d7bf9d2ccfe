"""Image-based lighting without a GPU: properties of the fp64 restatement (tests/_ibl_ref.py) the GPU tests compare the
kernels with, and the argument checks of pano_nerf_amd.ibl that need no device."""
import numpy as np
import pytest
import torch

import _ibl_ref as ref


def table(H, W):
    """(dirs [H W, 3], omega [H W]) fp64 of an equirectangular probe in the project's convention (y up)."""
    phi = ((np.arange(H) + 0.5) / H * np.pi)[:, None]
    theta = (-(np.arange(W) + 0.5) / W * 2.0 * np.pi)[None, :]
    d = np.stack([np.sin(phi) * np.sin(theta), np.cos(phi) * np.ones_like(theta), np.sin(phi) * np.cos(theta)], -1)
    omega = np.sin(phi) * (2.0 * np.pi / W) * (np.pi / H) * np.ones((1, W))
    return d.reshape(-1, 3), omega.reshape(-1)


def units(seed, K):
    v = np.random.default_rng(seed).normal(size=(K, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("samples", [32, 64, 128])
def test_table_bounds(samples):
    """A > 0, B > 0 and A + B <= 1 (F0 = 1 reflects at most everything); max A + B = 0.99997, min B = 2.5e-4."""
    t = ref.brdf_lut(16, samples)
    A, B = t[..., 0], t[..., 1]
    assert t.shape == (16, 16, 2) and np.isfinite(t).all()
    assert (A > 0).all() and (B > 0).all()
    assert (A + B <= 1.0).all(), float((A + B).max())


# --------------------------------------------------------------------------------------------------- the prefilter
@pytest.mark.parametrize("roughness", [0.2, 0.5, 1.0])
def test_constant_probe_prefilters_to_the_constant(roughness):
    dirs, omega = table(8, 16)
    probes = np.broadcast_to(np.array([0.25, 1.0, 7.5])[None, :, None, None], (1, 3, 8, 16))
    out = ref.prefilter(probes, dirs, omega, units(0, 17), roughness)
    np.testing.assert_allclose(out, np.broadcast_to([0.25, 1.0, 7.5], out.shape), rtol=1e-14)


def test_roughness_one_is_the_cosine_weighted_mean():
    """alpha = 1: den = 1 and the weights are c omega, so the result is sum L c omega / sum c omega"""
    dirs, omega = table(8, 16)
    rng = np.random.default_rng(1)
    probes = rng.random((2, 3, 8, 16)) + 0.1
    n = units(2, 9)
    c = np.maximum(n @ dirs.T, 0.0)  # [K, HW]
    want = np.einsum("kx,pcx->pkc", c * omega[None], probes.reshape(2, 3, -1)) / (c * omega[None]).sum(-1)[None, :, None]
    np.testing.assert_allclose(ref.prefilter(probes, dirs, omega, n, 1.0), want, rtol=1e-12)


def test_a_sharp_lobe_follows_the_brightest_pixel():
    """one bright pixel: at low roughness the prefiltered value along its direction is far above the one at 90 degrees"""
    dirs, omega = table(16, 32)
    probes = np.full((1, 3, 16, 32), 0.01)
    pix = 5 * 32 + 7
    probes.reshape(1, 3, -1)[:, :, pix] = 100.0
    d = dirs[pix]
    side = np.cross(d, [0.0, 1.0, 0.0])
    side /= np.linalg.norm(side)
    out = ref.prefilter(probes, dirs, omega, np.stack([d, side]), 0.3)
    assert out[0, 0, 0] > 50.0 * out[0, 1, 0]


# -------------------------------------------------------------------------------------------------- the evaluation
def test_cube_lookup_inverts_the_face_table():
    """cube_pos sends the direction of face texel (x, y) back to (x + 1/2, y + 1/2) of that face"""
    S = 4
    x, y = np.meshgrid(np.arange(S) + 0.5, np.arange(S) + 0.5)
    s, t = (2.0 * x / S - 1.0).ravel(), (2.0 * y / S - 1.0).ravel()
    one = np.ones_like(s)
    faces = [(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one)]
    for f, d in enumerate(faces):
        face, px, py = ref.cube_pos(S, np.stack(d, -1))
        assert (face == f).all()
        np.testing.assert_allclose(px, x.ravel(), atol=1e-12)
        np.testing.assert_allclose(py, y.ravel(), atol=1e-12)


def test_constant_maps_shade_to_the_closed_form():
    S, Si, St = 8, 4, 8
    spec = [np.full((3, 6 * (S >> l), S >> l), 2.0) for l in range(3)]
    irr = np.full((3, 6 * Si, Si), 3.0)
    lut = ref.brdf_lut(St, 16)
    n, vd = units(3, 33), units(4, 33)
    albedo = np.random.default_rng(5).random((33, 3))
    rough = np.linspace(0.0, 1.0, 33)
    rgb, diffuse, specular = ref.ibl_shade(spec, irr, lut, albedo, n, vd, rough, f0=0.04)
    np.testing.assert_allclose(diffuse, albedo / np.pi * 3.0, rtol=1e-14)
    # the table's own bilinear value at (NoV, roughness)
    NoV = np.maximum(-(n * vd).sum(-1), 0.0)
    xi, tx = ref.cell(NoV * St - 0.5, St - 1)
    yi, ty = ref.cell(rough.astype(np.float32).astype(np.float64) * St - 0.5, St - 1)
    ab = ((1 - ty) * (1 - tx))[:, None] * lut[yi, xi] + ((1 - ty) * tx)[:, None] * lut[yi, xi + 1] + \
        (ty * (1 - tx))[:, None] * lut[yi + 1, xi] + (ty * tx)[:, None] * lut[yi + 1, xi + 1]
    np.testing.assert_allclose(specular, (2.0 * (np.float64(np.float32(0.04)) * ab[:, 0] + ab[:, 1]))[:, None] * np.ones(3), rtol=1e-12)
    np.testing.assert_allclose(rgb, diffuse + specular, rtol=1e-15)


# ------------------------------------------------------------------------------------------------ argument checks
def test_arguments_are_checked_without_a_device():
    from pano_nerf_amd import ibl
    probes = torch.ones(1, 3, 8, 16)
    n = torch.tensor([[0.0, 1.0, 0.0]])
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="roughness"):
            ibl.prefilter(probes, n, bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ibl.prefilter(probes, n, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ibl.irradiance_cubemaps(probes, 4)
    for size in (3, 12, 2, 0, 8.5):
        with pytest.raises(ValueError, match="power of two"):
            ibl.prefilter_cubemaps(probes, size)
    for levels in (1, 0, 5, 2.5):  # size 8: 2 .. 4
        with pytest.raises(ValueError, match="levels"):
            ibl.prefilter_cubemaps(probes, 8, levels)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ibl.prefilter_cubemaps(probes, 8, 4)
    with pytest.raises(ValueError, match="probes must be"):
        ibl.prefilter(torch.ones(3, 8, 16), n, 0.5)
    for kw in (dict(size=1), dict(size=5000), dict(samples=0), dict(samples=2.5)):
        with pytest.raises(ValueError):
            ibl.brdf_lut(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ibl.brdf_lut(8, 8, device="cpu")
    with pytest.raises(ValueError, match="bake_ibl"):
        ibl.ibl_shade((1, 2, 3, 4), n, n, n, 0.5)
    cpu = ibl.IBL([torch.ones(1, 3, 24, 4), torch.ones(1, 3, 12, 2)], (0.0, 1.0), torch.ones(1, 3, 12, 2), torch.ones(4, 4, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ibl.ibl_shade(cpu, n, n, n, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ibl.save_ibl(cpu, "unused")


def test_the_package_exports_the_module():
    import pano_nerf_amd as pn
    from pano_nerf_amd import _lib
    assert pn.ibl.IBL._fields == ("specular", "roughness", "irradiance", "lut")
    assert pn.ibl.FACES == ("+x", "-x", "+y", "-y", "+z", "-z")
    for name in ("pn_prefilter_work_doubles", "pn_prefilter", "pn_brdf_lut", "pn_ibl_shade"):
        assert name in _lib.SIGNATURES
