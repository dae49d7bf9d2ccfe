"""Geometry export on the GPU: the marching-tetrahedra kernels against the numpy restatement of the contract
(test_geometry_cpu.py), the geometry of an analytic sphere, field queries against the fp64 oracle, grid / chunk
consistency and extract_mesh end to end."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_geometry_spec", os.path.join(os.path.dirname(__file__), "test_geometry_cpu.py"))
spec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spec)

BOX = spec.BOX


def dev():
    return torch.device("cuda:0")


def mt(sigma, level, bounds=None):
    from pano_nerf_amd import geometry
    v, f = geometry.marching_tetrahedra(torch.from_numpy(sigma).to(dev()), level, bounds)
    torch.cuda.synchronize()
    return v.cpu().numpy(), f.cpu().numpy()


def noise_field(res, seed):
    return np.random.default_rng(seed).normal(size=res).astype(np.float32)


@pytest.mark.parametrize("name", ["noise", "noise_box", "sphere33", "at_level", "all_inside", "all_outside", "nan"])
def test_kernels_match_the_spec(name):
    bounds = None
    if name == "noise":
        s, level = noise_field((9, 7, 5), 0), 0.0
    elif name == "noise_box":
        s, level, bounds = noise_field((9, 7, 5), 1), 0.3, ((-0.5, 0.25, 1.0), (1.5, 0.75, 3.0))
    elif name == "sphere33":
        s, level, bounds = spec.sphere_field((33, 33, 33)), 0.0, BOX
    elif name == "at_level":  # many values exactly at the level (outside: strict >)
        s, level = np.round(noise_field((12, 10, 11), 2)).astype(np.float32), 0.0
    elif name == "all_inside":
        s, level = np.ones((6, 5, 4), np.float32), 0.5
    elif name == "all_outside":
        s, level = np.zeros((6, 5, 4), np.float32), 0.5
    else:
        s, level = noise_field((10, 9, 8), 3), 0.0
        s[np.random.default_rng(4).random(s.shape) < 0.05] = np.nan  # NaN is outside
    v, f = mt(s, level, bounds)
    rv, rf, _ = spec.mt_reference(s, level, bounds)
    assert v.shape == rv.shape and f.shape == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    np.testing.assert_array_equal(f, rf)
    ok = np.isfinite(rv)
    assert np.array_equal(ok, np.isfinite(v))
    if len(rv):
        lo, step = spec.placement(s.shape, bounds)
        extent = float(np.max(np.abs(step) * (np.asarray(s.shape) - 1)))
        assert np.max(np.abs(v[ok] - rv[ok])) <= 1e-6 * extent
    if name in ("all_inside", "all_outside"):
        assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == np.int32


def test_sphere_geometry_and_determinism():
    res, R = (128, 128, 128), 0.6
    s = spec.sphere_field(res, R)
    v, f = mt(s, 0.0, BOX)
    v2, f2 = mt(s, 0.0, BOX)
    assert np.array_equal(v.view(np.uint32), v2.view(np.uint32)) and np.array_equal(f, f2)
    und, dirc = spec.edge_stats(f)
    assert np.all(und == 2) and np.all(dirc == 1)
    assert spec.euler(v, f) == 2
    a, b, c = (v[f[:, q]].astype(np.float64) for q in range(3))
    n = np.cross(b - a, c - a)
    area2 = np.linalg.norm(n, axis=1)
    big = area2 > 1e-9 * area2.max()
    assert np.all(np.einsum("ij,ij->i", n, (a + b + c) / 3)[big] > 0)
    area = 0.5 * area2.sum()
    volume = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0  # divergence theorem
    assert abs(area / (4 * np.pi * R ** 2) - 1) < 0.01, area
    assert abs(volume / (4 / 3 * np.pi * R ** 3) - 1) < 0.01, volume


def test_grid_points_placement():
    from pano_nerf_amd import geometry
    bounds, res = ((-0.7, 0.1, -2.0), (0.9, 1.3, 0.5)), (7, 5, 9)
    mean, cov = geometry.grid_points(bounds, res, variance=0.01)
    want = spec.grid_coords(res, bounds).reshape(-1, 3)
    np.testing.assert_array_equal(mean.cpu().numpy(), want)
    assert np.all(cov.cpu().numpy() == np.float32(0.01))


# ------------------------------------------------------------------------------------------------ field vs oracle
def make_model(cls, mode, nc, **kw):
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    extra = dict(mlp_num_density_channels=5, num_env_samples=10) if cls == "pano" else {}
    model = (pn.PanoMipNeRF if cls == "pano" else pn.MipNeRF)(num_samples=16, rgb_activation="softplus", **extra, **kw)
    params = orc.init_params(4, nc)
    model.mlp.load_state_dict(params)
    model = model.to(dev())
    model.mlp_mode = mode
    return model, params


def min_gate_margin(p, mean, cov, viewdirs):
    """min |pre-activation| over every ReLU of the oracle MLP, per point (fp64): a gate this close to zero may flip under
    fp32 rounding, which moves d sigma / d mean discontinuously (sigma itself is continuous)."""
    from oracle import pano_oracle as orc
    enc = orc.integrated_pos_enc(mean, cov, 0, 16)
    venc = orc.pos_enc(viewdirs, 0, 4)
    x, m = enc, torch.full(mean.shape[:-1], float("inf"), dtype=torch.float64)
    lin = torch.nn.functional.linear
    for i in range(8):
        z = lin(x, p[f"layers.{i}.0.weight"], p[f"layers.{i}.0.bias"])
        m = torch.minimum(m, z.abs().amin(-1))
        x = torch.relu(z)
        if i % 4 == 0 and i > 0:
            x = torch.cat([x, enc], -1)
    bott = lin(x, p["extra_layer.weight"], p["extra_layer.bias"])
    ve = venc[:, None, :].expand(-1, enc.shape[1], -1)
    z = lin(torch.cat([bott, ve], -1), p["view_layers.0.0.weight"], p["view_layers.0.0.bias"])
    return torch.minimum(m, z.abs().amin(-1))[:, 0]


def oracle_field(params, pts, var, vd, model, autocast=False, dt=torch.float64):
    from oracle import pano_oracle as orc
    dt = torch.float32 if autocast else dt
    p = {k: v.to(dt) for k, v in params.items()}
    mean, cov = pts.to(dt)[:, None, :], var.to(dt)[:, None, :]
    kw = dict(rgb_padding=model.rgb_padding, density_bias=model.density_bias)
    ctx = torch.autocast("cpu", dtype=torch.bfloat16) if autocast else torch.autocast("cpu", enabled=False)
    with ctx:
        with torch.no_grad():
            rgb, sigma, albedo = orc.radiance_field(p, mean, cov, vd.to(dt), **kw)
        grad = -orc.density_normals(p, mean, cov, vd.to(dt), **kw).detach()
    out = {"sigma": sigma[:, 0, 0], "rgb": rgb[:, 0], "grad": grad[:, 0]}
    if albedo is not None:
        out["albedo"] = albedo[:, 0]
    out = {k: v.double().numpy() for k, v in out.items()}
    out["margin"] = min_gate_margin(p, mean, cov, vd.to(dt)).double().numpy() if not autocast else None
    return out


CASES = [("pano", "fused_f16x2", 5, {}), ("pano", "fused", 5, {}), ("pano", "layerwise", 5, {}),
         ("pano", "fused_bf16", 5, {}), ("mip", "fused_f16x2", 1, {}), ("pano", "fused_f16x2", 5, {"disable_integration": True})]


@pytest.mark.parametrize("cls,mode,nc,kw", CASES, ids=["f16x2", "fused", "layerwise", "bf16", "mip", "no_integration"])
def test_query_field_against_the_oracle(cls, mode, nc, kw):
    from pano_nerf_amd import geometry
    model, params = make_model(cls, mode, nc, **kw)
    g = torch.Generator().manual_seed(11)
    M = 4096
    pts = torch.rand(M, 3, generator=g) * 3.0 - 1.5
    var = 10.0 ** (torch.rand(M, 3, generator=g) * 4.0 - 6.0)
    vd = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=-1)
    outs = ("sigma", "rgb", "normal", "grad") + (("albedo",) if nc == 5 else ())
    got = geometry.query_field(model, pts.to(dev()), var.to(dev()), viewdirs=vd.to(dev()), outputs=outs)
    got = {k: v.cpu().double().numpy() for k, v in got.items()}
    if kw.get("disable_integration"):
        var = torch.zeros_like(var)  # the model must ignore the variance it was given
    ref = oracle_field(params, pts, var, vd, model)
    stable = ref["margin"] > 1e-5  # grad / normal: points whose ReLU gates cannot flip under fp32 rounding
    assert stable.mean() > 0.8
    if mode == "fused_bf16":
        ref16 = oracle_field(params, pts, var, vd, model, autocast=True)
        for k in ("sigma", "rgb", "albedo", "grad"):
            if k not in got:
                continue
            scale = max(float(np.abs(ref[k]).max()), 1e-30)
            ours = float(np.abs(got[k] - ref[k]).max()) / scale
            theirs = float(np.abs(ref16[k] - ref[k]).max()) / scale
            assert ours <= 3 * theirs + 1e-3, (k, ours, theirs)
        return
    tol_grad = 1e-4
    if kw.get("disable_integration"):
        # zero covariance: plain PE up to 2^15 x, whose fp32 argument rounding alone moves d sigma / d mean by percents of
        # its max - the fp32 oracle is as far from the fp64 one.  Ours may deviate 3x as much as the fp32 oracle (+1e-4)
        ref32 = oracle_field(params, pts, var, vd, model, dt=torch.float32)
        scale = max(float(np.abs(ref["grad"]).max()), 1e-30)
        tol_grad += 3 * float(np.abs(ref32["grad"] - ref["grad"])[stable].max()) / scale
    for k in ("sigma", "rgb", "albedo", "grad"):
        if k not in got:
            continue
        sel = stable if k == "grad" else slice(None)
        scale = max(float(np.abs(ref[k]).max()), 1e-30)
        err = float(np.abs(got[k][sel] - ref[k][sel]).max()) / scale
        assert err <= (tol_grad if k == "grad" else 1e-4), (k, err, tol_grad)
    gn = np.linalg.norm(ref["grad"], axis=1)
    big = stable & (gn > 1e-3 * gn.max())
    n_ref = -ref["grad"][big] / gn[big, None]
    # |d n| <= |d g| / |g| (twice for the normalisation), with the grad's tolerance (of its max)
    tol = 2 * tol_grad * gn.max() / gn[big] + 1e-6
    assert np.all(np.linalg.norm(got["normal"][big] - n_ref, axis=1) <= tol)


# ------------------------------------------------------------------------------------------------ grids and meshes
def test_density_grid_matches_query_field_and_chunking():
    from pano_nerf_amd import geometry
    model, _ = make_model("pano", "fused_f16x2", 5)
    bounds, res = ((-1.2, -0.9, -1.0), (1.0, 1.1, 0.8)), (37, 29, 33)
    vol = geometry.density_grid(model, bounds, res)
    assert vol.shape == res and vol.is_contiguous() and vol.dtype == torch.float32
    step = [(h - l) / (n - 1) for l, h, n in zip(*bounds, res)]
    var = float(np.float32(max(float(np.float32(s)) for s in step) ** 2 / 12.0))
    mean, cov = geometry.grid_points(bounds, res, variance=var)
    q = geometry.query_field(model, mean, cov, outputs=("sigma",))["sigma"]
    assert torch.equal(vol.view(-1), q)
    for rows in (1000, 4096, 7777, 37 * 29 * 33):
        assert torch.equal(geometry.density_grid(model, bounds, res, chunk_rows=rows), vol), rows
    assert torch.equal(geometry.query_field(model, mean, cov, outputs=("sigma",), chunk_rows=999)["sigma"], q)


def test_extract_mesh_end_to_end(tmp_path):
    from oracle import pano_oracle as orc
    from pano_nerf_amd import geometry
    import pano_nerf_amd as pn
    _, _, _, c2ws = orc.synthetic_scene(8, 16, 3, seed=4)
    cams = np.stack([c[:3, 3] for c in c2ws])
    lo, hi = cams.min(0) - 1.0, cams.max(0) + 1.0
    bounds = (tuple(lo.tolist()), tuple(hi.tolist()))
    model, _ = make_model("pano", "fused_f16x2", 5)
    res, var = 40, 1e-4
    vol = geometry.density_grid(model, bounds, res, variance=var)
    level = float(torch.quantile(vol.view(-1)[::7].float(), 0.6))
    mesh = pn.extract_mesh(model, bounds, res, level, variance=var, chunk_rows=5000)
    v, f = geometry.marching_tetrahedra(vol, level, bounds)
    assert len(mesh.faces) > 100
    assert torch.equal(mesh.vertices, v) and torch.equal(mesh.faces, f)
    q = geometry.query_field(model, mesh.vertices, var, outputs=("normal", "albedo"))
    assert torch.equal(mesh.normals, q["normal"]) and torch.equal(mesh.colors, q["albedo"])
    # radiance colours: rgb seen along -normal
    mesh_r = pn.extract_mesh(model, bounds, res, level, variance=var, colors="radiance", normals=False)
    assert mesh_r.normals is None
    rgb = geometry.query_field(model, mesh.vertices, var, viewdirs=-q["normal"], outputs=("rgb",))["rgb"]
    assert torch.equal(mesh_r.colors, rgb)
    # topology: edges used by one face lie on the box boundary; interior directed edges are paired
    vn, fn = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    d = np.concatenate([fn[:, [0, 1]], fn[:, [1, 2]], fn[:, [2, 0]]]).astype(np.int64)
    dkey = d[:, 0] * (1 << 32) + d[:, 1]
    assert len(np.unique(dkey)) == len(dkey)  # every directed edge once
    und = np.sort(d, 1)
    k, cnt = np.unique(und[:, 0] * (1 << 32) + und[:, 1], return_counts=True)
    assert cnt.max() <= 2
    single = np.stack([k >> 32, k & 0xFFFFFFFF], 1)[cnt == 1]
    ends = vn[single.reshape(-1)].reshape(-1, 2, 3)
    lo32, hi32 = np.float32(lo), spec.grid_coords((res,) * 3, bounds)[-1, -1, -1]
    on = np.isclose(ends, lo32, atol=1e-5) | np.isclose(ends, hi32, atol=1e-5)
    assert np.all((on[:, 0] & on[:, 1]).any(-1))
    paired = set(dkey.tolist())
    interior = np.isin(und[:, 0] * (1 << 32) + und[:, 1], k[cnt == 2])
    assert all((int(b) << 32 | int(a)) in paired for a, b in d[interior])
    # PLY round trip
    path = str(tmp_path / "mesh.ply")
    geometry.write_ply(path, mesh.vertices, mesh.faces, mesh.normals, mesh.colors)
    names, vrec, faces = spec.read_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    np.testing.assert_array_equal(np.stack([vrec["x"], vrec["y"], vrec["z"]], 1), vn)
    np.testing.assert_array_equal(np.stack([vrec["nx"], vrec["ny"], vrec["nz"]], 1), mesh.normals.cpu().numpy())
    np.testing.assert_array_equal(faces, fn)


def test_empty_and_cpu_inputs():
    from pano_nerf_amd import geometry
    model, _ = make_model("pano", "fused_f16x2", 5)
    out = geometry.query_field(model, torch.zeros(0, 3, device=dev()), outputs=("sigma", "normal"))
    assert out["sigma"].shape == (0,) and out["normal"].shape == (0, 3)
    mesh = geometry.extract_mesh(model, BOX, 6, 1e9)
    assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3) and mesh.normals.shape == (0, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.query_field(model, torch.zeros(4, 3))
