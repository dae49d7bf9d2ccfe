"""Image-based lighting on the GPU: the prefilter, the BRDF table and ibl_shade against the fp64 restatement of
tests/_ibl_ref.py to one fp32 unit in the last place, the cube-map chain against the functions it is made of bit for
bit, orientation end to end, the exported files and the argument checks.

"<= 1 ulp" is |gpu - ref| <= np.spacing(|ref| as fp32): both sides do the same fp64 arithmetic on the same fp32 inputs,
their fp64 results differ by about H W eps64 at most, so the fp32 roundings can disagree only where that sliver
straddles a rounding boundary."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import _ibl_ref as ref

pytestmark = pytest.mark.gpu

SIZES = {"8x16": (8, 16), "18x36": (18, 36), "24x48": (24, 48), "32x64": (32, 64)}  # < 1 tile; ragged tile; 2 segments,
P = 3                                                                                # the last ragged; 2 even segments


def dev():
    return torch.device("cuda:0")


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def random_probes(n, H, W, seed):
    """[n, H, W, 3] strictly positive HDR radiance with a few bright pixels (CPU)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, H, W, 3, generator=g) * 2.0 + 0.05
    x[torch.rand(n, H, W, generator=g) < 0.01] *= 20.0
    return x


def layouts(x):
    x = x.to(dev())
    return {"phw3": x.permute(0, 3, 1, 2), "contiguous": x.permute(0, 3, 1, 2).contiguous()}


def unit(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(*shape, 3, generator=g, dtype=torch.float64)
    return (v / v.norm(dim=-1, keepdim=True)).to(torch.float32)


def tables(H, W):
    from pano_nerf_amd import lighting
    dirs, omega = lighting._table(H, W, dev())
    return dirs.cpu().numpy(), omega.cpu().numpy()


@functools.lru_cache(maxsize=None)
def prefilter_case(size, K, per_probe, roughness):
    """(probes [P, H, W, 3] CPU, directions CPU, restatement [P, K, 3]) - computed once, shared by both layouts"""
    H, W = SIZES[size]
    x = random_probes(P, H, W, seed=H + K)
    n = unit(K + int(per_probe), P, K) if per_probe else unit(K, K)
    want = ref.prefilter(x.permute(0, 3, 1, 2).numpy(), *tables(H, W), n.numpy(), roughness)
    return x, n, want


# ------------------------------------------------------------------------------------------------------ prefilter
@pytest.mark.parametrize("layout", ["phw3", "contiguous"])
@pytest.mark.parametrize("size", list(SIZES))
def test_prefilter_matches_the_restatement(size, layout):
    from pano_nerf_amd import ibl
    worst = 0.0
    for K in (1, 255, 257):
        for per_probe in (False, True):
            for roughness in (0.2, 0.5, 1.0):
                x, n, want = prefilter_case(size, K, per_probe, roughness)
                got = ibl.prefilter(layouts(x)[layout], n.to(dev()), roughness)
                assert tuple(got.shape) == (P, K, 3) and got.dtype == torch.float32
                ok, ratio = ref.ulp_ok(got.cpu().numpy(), want)
                worst = max(worst, ratio)
                assert ok, (size, layout, K, per_probe, roughness, ratio)
    print(f"prefilter {size} {layout}: worst |gpu - ref| = {worst:.3f} ulp")


@pytest.mark.parametrize("size", ["18x36", "32x64"])
def test_prefilter_does_not_depend_on_the_probe_count(size):
    from pano_nerf_amd import ibl
    H, W = SIZES[size]
    probes = layouts(random_probes(P, H, W, seed=7))["phw3"]
    shared, per = unit(1, 300).to(dev()), unit(2, P, 300).to(dev())
    full = ibl.prefilter(probes, shared, 0.4)
    assert bits_equal(ibl.prefilter(probes[1:2], shared, 0.4), full[1:2])
    assert bits_equal(ibl.prefilter(probes, shared, 0.4), full)
    full = ibl.prefilter(probes, per, 0.4)
    assert bits_equal(ibl.prefilter(probes[1:2], per[1:2], 0.4), full[1:2])
    assert bits_equal(ibl.prefilter(probes, shared[None], 0.4), ibl.prefilter(probes, shared, 0.4))


def test_roughness_one_agrees_with_irradiance():
    """alpha = 1: prefilter = E(L) / E(1), so prefilter E(1) = E(L) up to three fp32 roundings and one product: 4 ulp"""
    from pano_nerf_amd import ibl, lighting
    probes = layouts(random_probes(P, 18, 36, seed=11))["phw3"]
    n = unit(3, 257).to(dev())
    lhs = (ibl.prefilter(probes, n, 1.0) * lighting.irradiance(torch.ones_like(probes), n)).cpu().numpy().astype(np.float64)
    rhs = lighting.irradiance(probes, n).cpu().numpy()
    assert (np.abs(lhs - rhs) <= 4.0 * np.spacing(np.abs(rhs))).all()


def test_nan_radiance_poisons_its_channel_only():
    from pano_nerf_amd import ibl
    x = random_probes(2, 8, 16, seed=13)
    x[1, 3, 5, 2] = float("nan")
    got = ibl.prefilter(layouts(x)["phw3"], unit(4, 9).to(dev()), 0.5).cpu()
    assert torch.isnan(got[1, :, 2]).all() and torch.isfinite(got[1, :, :2]).all() and torch.isfinite(got[0]).all()


# ------------------------------------------------------------------------------------------------------- cube maps
@pytest.mark.parametrize("case", ["16x32-size8-levels3", "8x16-size4-levels2"])
def test_prefilter_cubemaps_is_made_of_its_parts(case):
    from pano_nerf_amd import ibl, lighting, views
    (H, W), size, levels = {"16x32-size8-levels3": ((16, 32), 8, 3), "8x16-size4-levels2": ((8, 16), 4, 2)}[case]
    probes = layouts(random_probes(2, H, W, seed=17))["phw3"]
    chain, rough = ibl.prefilter_cubemaps(probes, size, levels)
    assert len(chain) == levels and rough == tuple(l / (levels - 1) for l in range(levels))
    assert bits_equal(chain[0], lighting.probes_to_cubemaps(probes, size, 4))
    for l in range(1, levels):
        S = size >> l
        assert tuple(chain[l].shape) == (2, 3, 6 * S, S)
        n = views.generate_camera_rays(views.cubemap_camera(S), np.eye(4, dtype=np.float32), device=dev()).viewdirs
        want = ibl.prefilter(probes, n, rough[l]).view(2, 6 * S, S, 3).permute(0, 3, 1, 2)
        assert bits_equal(chain[l], want)
    irr = ibl.irradiance_cubemaps(probes, 4)
    n = views.generate_camera_rays(views.cubemap_camera(4), np.eye(4, dtype=np.float32), device=dev()).viewdirs
    assert bits_equal(irr, lighting.irradiance(probes, n).view(2, 24, 4, 3).permute(0, 3, 1, 2))


def test_default_levels_end_at_four_texels():
    from pano_nerf_amd import ibl
    chain, rough = ibl.prefilter_cubemaps(layouts(random_probes(1, 32, 64, seed=19))["phw3"], 32)
    assert [int(t.shape[3]) for t in chain] == [32, 16, 8, 4] and rough == (0.0, 1 / 3, 2 / 3, 1.0)


def test_the_resolution_guard():
    from pano_nerf_amd import ibl
    probes = layouts(random_probes(1, 16, 32, seed=23))["phw3"]
    with pytest.raises(ValueError, match="cannot resolve"):  # levels = 4, r_1 = 1/3: pi / 16 = 0.196 > 1/9
        ibl.prefilter_cubemaps(probes, 32)
    chain, _ = ibl.prefilter_cubemaps(probes, 32, allow_coarse=True)
    assert len(chain) == 4 and all(bool(torch.isfinite(t).all()) for t in chain)


# ------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("size,samples", [(8, 32), (16, 64)])
def test_brdf_lut_matches_the_restatement(size, samples):
    from pano_nerf_amd import ibl
    got = ibl.brdf_lut(size, samples, device=dev())
    assert tuple(got.shape) == (size, size, 2) and got.dtype == torch.float32
    ok, ratio = ref.ulp_ok(got.cpu().numpy(), ref.brdf_lut(size, samples))
    print(f"brdf_lut({size}, {samples}): worst |gpu - ref| = {ratio:.3f} ulp")
    assert ok, ratio
    assert bits_equal(got, ibl.brdf_lut(size, samples, device=dev()))


# -------------------------------------------------------------------------------------------------------- shading
@pytest.fixture(scope="module")
def baked():
    from pano_nerf_amd import ibl
    probes = layouts(random_probes(2, 16, 32, seed=29))["phw3"]
    return ibl.bake_ibl(probes, size=8, levels=3, irradiance_size=4, lut_size=8, lut_samples=32)


def test_bake_ibl_is_made_of_its_parts(baked):
    from pano_nerf_amd import ibl
    probes = layouts(random_probes(2, 16, 32, seed=29))["phw3"]  # the fixture's probes
    chain, rough = ibl.prefilter_cubemaps(probes, 8, 3)
    assert baked.roughness == rough and all(bits_equal(a, b) for a, b in zip(baked.specular, chain))
    assert bits_equal(baked.irradiance, ibl.irradiance_cubemaps(probes, 4))
    assert bits_equal(baked.lut, ibl.brdf_lut(8, 32, device=dev()))


def shade_rows(R, seed):
    """albedo, normals, viewdirs [R, 3] (CPU): random unit vectors, so about half the rows have n . v < 0; from 16 rows
    on, the first are axis and diagonal normals seen head-on (face ties in the lookup)."""
    g = torch.Generator().manual_seed(seed)
    albedo = torch.rand(R, 3, generator=g)
    n, vd = unit(seed + 1, R), unit(seed + 2, R) * (0.5 + torch.rand(R, 1, generator=g))  # viewdirs need no unit length
    if R >= 16:
        special = torch.tensor([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 1], [-1, 1, -1],
                                [1, 1, 0], [0, -1, -1]], dtype=torch.float64)
        special = (special / special.norm(dim=-1, keepdim=True)).to(torch.float32)
        n[:10] = special
        vd[:10] = -special
    return albedo, n, vd


@pytest.mark.parametrize("roughness", ["0", "0.37", "1", "per-row"])
@pytest.mark.parametrize("R", [1, 257])
def test_ibl_shade_matches_the_restatement(baked, R, roughness):
    from pano_nerf_amd import ibl
    albedo, n, vd = shade_rows(R, seed=31 + R)
    if roughness == "per-row":
        g = torch.Generator().manual_seed(37)
        rough = torch.rand(R, 1, generator=g)
        rough[:: 5] = 0.0
        rough[1:: 5] = 1.0
        rough[2:: 5] = 0.5  # exactly on level 1
        rough_dev = rough.to(dev())
    else:
        rough = rough_dev = float(roughness)
    assert R == 1 or bool(((n * -vd).sum(-1) < 0).any())
    got = ibl.ibl_shade(baked, albedo.to(dev()), n.to(dev()), vd.to(dev()), rough_dev, f0=0.04, probe=1)
    want = ref.ibl_shade([t[1].cpu().numpy() for t in baked.specular], baked.irradiance[1].cpu().numpy(),
                         baked.lut.cpu().numpy(), albedo.numpy(), n.numpy(), vd.numpy(),
                         rough.numpy().reshape(-1) if roughness == "per-row" else rough, f0=0.04)
    for name, g_, w_ in zip(("rgb", "diffuse", "specular"), got, want):
        assert tuple(g_.shape) == (R, 3) and g_.dtype == torch.float32
        ok, ratio = ref.ulp_ok(g_.cpu().numpy(), w_)
        assert ok, (name, R, roughness, ratio)


def test_orientation_end_to_end():
    """one pixel of value 100: the brightest level-0 texel looks along it, a mirror looking along it sees it, and the
    seven other octants see nothing"""
    from pano_nerf_amd import ibl, lighting, views
    H, W, S, i, j = 16, 32, 16, 5, 3
    x = torch.zeros(1, H, W, 3)
    x[0, i, j] = 100.0
    baked = ibl.bake_ibl(layouts(x)["phw3"], size=S, irradiance_size=4, lut_size=8, lut_samples=32)
    d = lighting._table(H, W, dev())[0][i * W + j].cpu().double()
    assert float(d.abs().min()) > 0.4  # every component is large: the other octants are far away
    texels = views.generate_camera_rays(views.cubemap_camera(S), np.eye(4, dtype=np.float32), device=dev()).viewdirs
    level0 = baked.specular[0][0].permute(1, 2, 0).reshape(-1, 3).cpu()
    brightest = texels[int(level0[:, 0].argmax())].cpu().double()
    # a texel spans at most 2 / S radians; the texel nearest the peak of the pixel's bilinear tent is the brightest
    assert float(torch.acos(torch.clamp((brightest * d).sum(), -1, 1))) <= 2.0 / S
    signs = torch.tensor([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], dtype=torch.float64)
    n = (signs * d).to(torch.float32)  # normal = mirror direction, seen head-on: Rr = n
    rgb, diffuse, spec = ibl.ibl_shade(baked, torch.zeros(8, 3).to(dev()), n.to(dev()), (-n).to(dev()), 0.0, f0=0.04)
    lut = baked.lut.cpu().double()
    scale = float(np.float32(0.04)) * float(lut[0, -1, 0]) + float(lut[0, -1, 1])  # NoV = 1, roughness 0: the last column of row 0
    light = spec.cpu().double() / scale
    # the fetch averages the pixel's tent (peak 100 at d) over at most +-1.5 texels = +-1.1 probe pixels around d, with
    # weights that fall off from the centre: more than the uniform mean of a tent over +-1 pixel, 100 / 4, less 20 % slack
    assert 20.0 < float(light[0].min()) and float(light[0].max()) <= 100.0 * (1 + 1e-6)
    assert bool((spec[1:] == 0).all()) and bool((diffuse == 0).all()) and bits_equal(rgb, spec)


def test_constant_probe():
    """specular = c (f0 A + B) and diffuse = albedo c sum omega max(0, n . d) / pi for any normal and roughness"""
    from pano_nerf_amd import ibl, lighting
    H, W, R = 16, 32, 64
    c = torch.tensor([0.5, 2.0, 8.0])
    x = c.expand(1, H, W, 3).contiguous()
    baked = ibl.bake_ibl(layouts(x)["phw3"], size=8, levels=3, irradiance_size=4, lut_size=8, lut_samples=32)
    albedo, n, vd = shade_rows(R, seed=41)
    rough = torch.rand(R, 1, generator=torch.Generator().manual_seed(43))
    _, diffuse, spec = ibl.ibl_shade(baked, albedo.to(dev()), n.to(dev()), vd.to(dev()), rough.to(dev()), f0=0.04)
    # specular: every level is c up to the fp32 roundings of level 0's resampling (4 products, 3 sums, a 16-term mean
    # and a quotient: below 24 roundings of 6e-8) - the filtered levels are c to an ulp
    zero = np.zeros((3, 6, 1))
    unit_light = ref.ibl_shade([np.ones((3, 6 * s, s)) for s in (8, 4, 2)], zero, baked.lut.cpu().numpy(), albedo.numpy(),
                               n.numpy(), vd.numpy(), rough.numpy().reshape(-1), f0=0.04)[2]
    np.testing.assert_allclose(spec.cpu().numpy(), unit_light * c.numpy()[None], rtol=24 * 6e-8)
    # diffuse: E(n) = sum omega max(0, n . d) is the midpoint rule for pi; the cube interpolates E between its texel
    # directions.  With eps the rule's largest error over the texel directions and the normals used, both sides lie
    # within eps of pi, so they differ by 2 eps at most.
    texels = ibl._texel_directions(4, dev())
    ones = torch.ones(1, 3, H, W, device=dev())
    e_texel = lighting.irradiance(ones, texels)[0, :, 0].cpu().double()
    e_n = lighting.irradiance(ones, n.to(dev()))[0, :, 0].cpu().double()
    eps = float(torch.cat([e_texel, e_n]).sub(np.pi).abs().max())
    assert eps < 0.05 * np.pi  # the rule is a rule for pi
    want = albedo.double() * c.double()[None] * e_n[:, None] / np.pi
    bound = albedo.double() * c.double()[None] * (2 * eps / np.pi) + 1e-6 * want
    assert bool(((diffuse.cpu().double() - want).abs() <= bound).all())


# --------------------------------------------------------------------------------------------------------- export
def test_save_ibl_reads_back(baked, tmp_path):
    from pano_nerf_amd import ibl, io_exr
    path = ibl.save_ibl(baked, str(tmp_path / "ibl"), probe=1)
    meta = json.load(open(path))
    assert meta["faces"] == ["+x", "-x", "+y", "-y", "+z", "-z"] and meta["probe"] == 1
    assert [lv["size"] for lv in meta["specular"]] == [8, 4, 2] and [lv["roughness"] for lv in meta["specular"]] == [0.0, 0.5, 1.0]
    files = [lv["file"] for lv in meta["specular"]] + [meta["irradiance"]["file"], meta["brdf_lut"]["file"]]
    assert sorted(files + ["ibl.json"]) == sorted(os.listdir(tmp_path / "ibl"))
    for lv, t in zip(meta["specular"], baked.specular):
        back = io_exr.read_exr(str(tmp_path / "ibl" / lv["file"]))
        assert bits_equal(torch.from_numpy(back), t[1].permute(1, 2, 0))
    assert bits_equal(torch.from_numpy(io_exr.read_exr(str(tmp_path / "ibl" / "irradiance.exr"))), baked.irradiance[1].permute(1, 2, 0))
    lut = io_exr.read_exr(str(tmp_path / "ibl" / "brdf_lut.exr"))
    assert meta["irradiance"]["size"] == 4 and meta["brdf_lut"]["size"] == 8
    assert bits_equal(torch.from_numpy(lut[:, :, :2].copy()), baked.lut) and not lut[:, :, 2].any()


# ------------------------------------------------------------------------------------------------------ bad input
def test_bad_input(baked):
    from pano_nerf_amd import ibl
    probes = layouts(random_probes(1, 16, 32, seed=47))["phw3"]
    n = unit(5, 4).to(dev())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ibl.prefilter(probes.cpu(), n, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ibl.prefilter(probes, n.cpu(), 0.5)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="roughness"):
            ibl.prefilter(probes, n, bad)
    with pytest.raises(ValueError, match="do not match"):
        ibl.prefilter(probes, unit(6, 2, 4).to(dev()), 0.5)
    with pytest.raises(ValueError, match="power of two"):
        ibl.prefilter_cubemaps(probes, 12)
    for levels in (1, 5):
        with pytest.raises(ValueError, match="levels"):
            ibl.prefilter_cubemaps(probes, 8, levels)
    for probe in (2, -1):
        with pytest.raises(IndexError, match="out of range"):
            ibl.ibl_shade(baked, n, n, n, 0.5, probe=probe)
        with pytest.raises(IndexError, match="out of range"):
            ibl.save_ibl(baked, "unused", probe=probe)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ibl.ibl_shade(baked, n.cpu(), n, n, 0.5)
    with pytest.raises(ValueError, match=r"\[R, 3\]"):
        ibl.ibl_shade(baked, n, n[:, :2], n, 0.5)
    with pytest.raises(ValueError, match="roughness"):
        ibl.ibl_shade(baked, n, n, n, torch.rand(3, 1, device=dev()))
