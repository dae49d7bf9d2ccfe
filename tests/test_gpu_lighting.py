"""Spatially-varying lighting on the GPU: probe conventions against the reference, probes against the renderer bit for
bit, the SH / quadrature kernels against the fp64 restatement of test_lighting_cpu.py, field_irradiance against the
renderer's shading bit for bit, the SH irradiance volume, and argument checks."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_lighting_spec", os.path.join(os.path.dirname(__file__), "test_lighting_cpu.py"))
spec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spec)

MODES = ("fused_f16x2", "fused_f16x2_t32", "fused", "fused_bf16", "layerwise")


def dev():
    return torch.device("cuda:0")


def make_model(cls, mode, **kw):
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    extra = dict(mlp_num_density_channels=5, num_env_samples=10) if cls == "pano" else {}
    model = (pn.PanoMipNeRF if cls == "pano" else pn.MipNeRF)(num_samples=16, rgb_activation="softplus", **extra, **kw)
    model.mlp.load_state_dict(orc.init_params(4, 5 if cls == "pano" else 1))
    model = model.to(dev())
    model.mlp_mode = mode
    return model


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))


def random_probes(P, H, W, seed, layout="phw3"):
    """[P, 3, H, W] HDR radiance: a permuted view of [P, H, W, 3] ("phw3", how light_probes returns probes) or contiguous."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(P, H, W, 3, generator=g) * 2.0
    x[torch.rand(P, H, W, generator=g) < 0.01] *= 20.0
    x = x.to(dev())
    return x.permute(0, 3, 1, 2) if layout == "phw3" else x.permute(0, 3, 1, 2).contiguous()


def unit(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(*shape, 3, generator=g, dtype=torch.float64)
    return (v / v.norm(dim=-1, keepdim=True)).to(torch.float32).to(dev())


# ------------------------------------------------------------------------------------------------------- conventions
@pytest.mark.parametrize("size", ["8x16", "16x32"])
def test_probe_directions_match_the_reference(size):
    from pano_nerf_amd import lighting
    g = load_golden("lighting_ref")
    H, W = (int(s) for s in size.split("x"))
    dirs, omega = lighting.probe_directions(H, W, dev())
    np.testing.assert_allclose(dirs.cpu().numpy(), g[size + "/dirs"], rtol=2e-6, atol=2e-7)
    assert np.array_equal(omega.cpu().numpy(), g[size + "/omega"])


# ------------------------------------------------------------------------------------------------------ probes
@pytest.mark.parametrize("mode", MODES)
def test_probes_are_the_rendered_panorama(mode):
    import pano_nerf_amd as pn
    from pano_nerf_amd import lighting
    H, W = 16, 32
    pos = np.array([[0.1, -0.2, 0.3], [-0.4, 0.25, 0.05]], np.float32)
    model = make_model("pano", mode)
    probes = lighting.light_probes(model, torch.from_numpy(pos).to(dev()), H, W, chunk_rays=H * W)
    assert probes.shape == (2, 3, H, W) and probes.permute(0, 2, 3, 1).is_contiguous()
    for p in range(2):
        c2w = np.eye(4, dtype=np.float32)
        c2w[:3, 3] = pos[p]
        rays = pn.generate_pano_rays(H, W, c2w)
        env = pn.generate_lit_rays(10, pn.rays.pano_pixel_radius(rays))
        img = pn.render_image(model, pn.Rays(*[x.view(1, H, W, -1) for x in rays]), env, H, W, chunk_size=H * W)
        assert bits_equal(probes[p], img[1][0]), (mode, p)
    # MipNeRF: the level-1 rgb of its forward
    mip = make_model("mip", mode)
    mp = lighting.light_probes(mip, torch.from_numpy(pos).to(dev()), H, W, chunk_rays=H * W)
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = pos[1]
    rays = pn.generate_pano_rays(H, W, c2w)
    with torch.no_grad():
        out = mip(rays=rays, randomized=False, white_bkgd=False, use_ort_loss=False)
    assert bits_equal(mp[1], out[1][0].view(H, W, 3).permute(2, 0, 1)), mode
    assert bool(torch.isfinite(probes).all()) and bool(torch.isfinite(mp).all())


def test_probe_chunking_is_invisible():
    from pano_nerf_amd import lighting
    model = make_model("pano", "fused_f16x2")
    pos = torch.tensor([[0.1, -0.2, 0.3], [-0.4, 0.25, 0.05], [0.0, 0.0, 0.0]], device=dev())
    a = lighting.light_probes(model, pos, 16, 32, chunk_rays=512)
    b = lighting.light_probes(model, pos, 16, 32, chunk_rays=700)
    c = lighting.light_probes(model, pos, 16, 32)
    assert bits_equal(a, b) and bits_equal(a, c)


# ------------------------------------------------------------------------------------------ SH and quadrature kernels
@pytest.mark.parametrize("size,layout", [("32x64", "phw3"), ("32x64", "contiguous"), ("128x256", "phw3")])
def test_sh_project_and_irradiance_match_the_restatement(size, layout):
    from pano_nerf_amd import lighting
    H, W = (int(s) for s in size.split("x"))
    P, K = 3, 40
    probes = random_probes(P, H, W, seed=H, layout=layout)
    dirs, omega = (t.cpu().numpy() for t in lighting.probe_directions(H, W, dev()))
    L = spec.as_pixels(probes.cpu().numpy())
    sh = lighting.sh_project(probes)
    assert sh.shape == (P, 9, 3)
    assert rel(sh.cpu().numpy(), spec.sh_project(L, dirs, omega)) < 1e-6
    shared, per = unit(1, K), unit(2, P, K)
    for n in (shared, shared[None], per):
        got = lighting.irradiance(probes, n)
        want = spec.irradiance_exact(L, n.cpu().numpy()[None] if n.dim() == 2 else n.cpu().numpy(), dirs, omega)
        assert got.shape == (P, K, 3)
        e = np.abs(got.cpu().numpy() - want) / np.maximum(np.abs(want), 1e-30)
        assert float(e.max()) < 1e-6, (size, layout, float(e.max()))
    # repeated calls give the same bits
    assert bits_equal(sh, lighting.sh_project(probes))
    assert bits_equal(lighting.irradiance(probes, per), lighting.irradiance(probes, per))


@pytest.mark.parametrize("size", ["8x16", "16x32"])
def test_irradiance_is_the_reference_shading(size):
    from pano_nerf_amd import lighting
    g = load_golden("lighting_ref")
    H, W = (int(s) for s in size.split("x"))
    env = torch.from_numpy(g[size + "/env"]).to(dev())  # [B, H W, 3]
    probes = env.view(-1, H, W, 3).permute(0, 3, 1, 2)
    n = torch.from_numpy(g[size + "/normal"]).to(dev())[:, None]  # one normal per probe
    got = lighting.irradiance(probes, n)[:, 0].cpu().numpy()
    np.testing.assert_allclose(got, g[size + "/shading"], rtol=2e-6, atol=1e-6 * np.abs(got).max())


def test_nan_pixel_propagates():
    from pano_nerf_amd import lighting
    probes = random_probes(2, 8, 16, seed=5, layout="contiguous")
    probes[1, 0, 3, 4] = float("nan")
    sh = lighting.sh_project(probes).cpu()
    e = lighting.irradiance(probes, unit(3, 6)).cpu()
    assert bool(torch.isnan(sh[1, :, 0]).all()) and bool(torch.isfinite(sh[0]).all()) and bool(torch.isfinite(sh[1, :, 1:]).all())
    assert bool(torch.isnan(e[1, :, 0]).all()) and bool(torch.isfinite(e[0]).all())


def test_sh_irradiance_matches_the_restatement_and_the_quadrature():
    from pano_nerf_amd import lighting
    H, W = 64, 128
    dirs_t, omega_t = lighting.probe_directions(H, W, dev())
    dirs = dirs_t.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(7)
    coef = rng.standard_normal((2, 9, 3))
    coef[:, 0] = 4.0
    L = np.einsum("nk,pkc->pnc", spec.sh_basis(dirs), coef).astype(np.float32)  # band-limited radiance
    probes = torch.from_numpy(L).to(dev()).view(2, H, W, 3).permute(0, 3, 1, 2)
    n = unit(8, 2, 32)
    sh = lighting.sh_project(probes)
    got = lighting.sh_irradiance(sh, n)
    want = spec.sh_irradiance(sh.cpu().numpy(), n.cpu().numpy())
    assert got.shape == (2, 32, 3) and rel(got.cpu().numpy(), want) < 1e-6
    shared = lighting.sh_irradiance(sh, n[0])
    assert rel(shared.cpu().numpy(), spec.sh_irradiance(sh.cpu().numpy(), n[:1].cpu().numpy())) < 1e-6
    exact = lighting.irradiance(probes, n).cpu().numpy()
    assert rel(got.cpu().numpy(), exact) < 3e-3  # quadrature error only


# ---------------------------------------------------------------------------------------- the field's own estimate
def _shading_chunk(model, env, B=256):
    import pano_nerf_amd as pn
    rays = pn.generate_pano_rays(16, 32, np.eye(4, dtype=np.float32))
    rays = pn.Rays(*[x[:B] for x in rays])
    with torch.no_grad():
        out = model(rays=rays, env_rays=env, randomized=False, white_bkgd=False, enable_surf=True, use_ort_loss=False)
    o, d = rays.origins, rays.directions
    dist, normal, shading = out[1][1], out[1][3], out[1][8]
    return o + d * dist.view(-1, 1), normal, shading


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("disint", [False, True])
def test_field_irradiance_is_the_renderer_shading(mode, disint):
    import pano_nerf_amd as pn
    from pano_nerf_amd import lighting
    model = make_model("pano", mode, disable_integration=disint)
    env = pn.generate_lit_rays(10, 0.01)
    pts, normal, shading = _shading_chunk(model, env)
    got = lighting.field_irradiance(model, pts, normal, env)
    assert bits_equal(got, shading), (mode, disint, rel(got.cpu().numpy(), shading.cpu().numpy()))


@pytest.mark.parametrize("mode", MODES)
def test_field_irradiance_mipnerf_chunks(mode):
    import pano_nerf_amd as pn
    from pano_nerf_amd import lighting
    model = make_model("mip", mode)
    env = pn.generate_lit_rays(10, 0.01)
    g = torch.Generator().manual_seed(11)
    pts = ((torch.rand(300, 3, generator=g) - 0.5) * 2.0).to(dev())
    n = unit(12, 300)
    a = lighting.field_irradiance(model, pts, n, env)
    b = lighting.field_irradiance(model, pts, n, env)
    assert a.shape == (300, 3) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    assert bits_equal(a, b)
    d = lighting.field_irradiance(model, pts, n, env, chunk_points=64)  # 64, 64, 64, 64, 44 points
    assert bits_equal(a, d), (mode, rel(d.cpu().numpy(), a.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ irradiance volume
def test_irradiance_volume():
    from pano_nerf_amd import geometry, lighting
    model = make_model("pano", "fused_f16x2")
    bounds, res = ((-0.5, -0.25, -0.5), (0.5, 0.25, 0.5)), (3, 2, 3)
    vol = lighting.irradiance_volume(model, bounds, res, 8, 16)
    assert vol.sh.shape == (3, 2, 3, 9, 3)
    lo, step = np.array(vol.lo), np.array(vol.step)
    verts_t, _ = geometry.grid_points(bounds, res)  # the vertices as the kernels place them
    verts = verts_t.cpu().numpy()
    want = lighting.sh_project(lighting.light_probes(model, verts_t, 8, 16))
    assert bits_equal(vol.sh.reshape(-1, 9, 3), want)
    sh = vol.sh.reshape(-1, 9, 3)
    n = unit(13, verts.shape[0])
    at_v = lighting.sample_irradiance(vol, verts_t, n)
    ref_v = lighting.sh_irradiance(sh, n[:, None])[:, 0]
    assert rel(at_v.cpu().numpy(), ref_v.cpu().numpy()) < 1e-6
    g = vol.sh.cpu().numpy()
    # cell centres: the mean of the eight corners
    cells = np.array([[0, 0, 0], [1, 0, 1], [0, 0, 1]])
    centres = (lo + (cells + 0.5) * step).astype(np.float32)
    nc = unit(14, len(cells))
    got = lighting.sample_irradiance(vol, torch.from_numpy(centres).to(dev()), nc).cpu().numpy()
    mean = np.stack([np.mean([g[a + x, b + y, c + z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], 0)
                     for a, b, c in cells])
    want_c = np.einsum("mj,mjc->mc", spec.sh_basis(nc.cpu().numpy()) * spec.A_HAT, mean)
    assert rel(got, want_c) < 1e-6
    assert rel(got, spec.volume_irradiance(g, lo, step, centres, nc.cpu().numpy())) < 1e-6
    # outside the box: clamped to the nearest face / corner
    outside = torch.tensor([[-3.0, 5.0, 0.1], [2.0, -2.0, 2.0]], device=dev())
    clamped = torch.maximum(torch.minimum(outside, torch.tensor(bounds[1], device=dev())),
                            torch.tensor(bounds[0], device=dev()))
    no = unit(15, 2)
    assert rel(lighting.sample_irradiance(vol, outside, no).cpu().numpy(),
               lighting.sample_irradiance(vol, clamped, no).cpu().numpy()) < 1e-6
    assert rel(lighting.sample_irradiance(vol, outside, no).cpu().numpy(),
               spec.volume_irradiance(g, lo, step, outside.cpu().numpy(), no.cpu().numpy())) < 1e-6


# ---------------------------------------------------------------------------------------------------- bad input
def test_bad_input_raises():
    import pano_nerf_amd as pn
    from pano_nerf_amd import lighting
    model = make_model("pano", "fused_f16x2")
    probes = random_probes(2, 8, 16, seed=1)
    n = unit(1, 4)
    env = pn.generate_lit_rays(10, 0.01)
    with pytest.raises(RuntimeError):
        lighting.sh_project(probes.cpu())
    with pytest.raises(RuntimeError):
        lighting.irradiance(probes, n.cpu())
    with pytest.raises(RuntimeError):
        lighting.light_probes(model, torch.zeros(1, 3))
    with pytest.raises(RuntimeError):
        lighting.field_irradiance(model, torch.zeros(4, 3), n.cpu(), env)
    with pytest.raises(RuntimeError):
        lighting.sh_irradiance(lighting.sh_project(probes).cpu(), n.cpu())
    with pytest.raises(ValueError):
        lighting.sh_project(probes[:, :2])
    with pytest.raises(ValueError):
        lighting.sh_project(torch.zeros(1, 3, 1, 16, device=dev()))
    with pytest.raises(ValueError):
        lighting.probe_directions(8, 1, dev())
    with pytest.raises(ValueError):
        lighting.light_probes(model, torch.zeros(1, 3, device=dev()), 1, 16)
    with pytest.raises(ValueError):
        lighting.irradiance(probes, unit(2, 3, 4))  # 3 normal sets for 2 probes
    with pytest.raises(ValueError):
        lighting.irradiance(probes, torch.zeros(4, 2, device=dev()))
    with pytest.raises(ValueError):
        lighting.sh_irradiance(torch.zeros(2, 4, 3, device=dev()), n)
    with pytest.raises(ValueError):
        lighting.field_irradiance(model, torch.zeros(4, 3, device=dev()), n[:3], env)
    with pytest.raises(ValueError):
        lighting.light_probes(model, torch.zeros(3, device=dev()))
    vol = lighting.IrradianceVolume(torch.zeros(1, 2, 2, 9, 3, device=dev()), (0.0,) * 3, (1.0,) * 3)
    with pytest.raises(ValueError):
        lighting.sample_irradiance(vol, torch.zeros(1, 3, device=dev()), n[:1])
