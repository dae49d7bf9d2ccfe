"""Virtual object insertion on the GPU: shade against the reference's own outputs, trace_mesh and shadow_ratio against the
fp64 restatement of test_objects_cpu.py, insert_object against the composition of its public pieces bit for bit, and
argument checks.  Tolerances: conftest.assert_close for the well-conditioned outputs; for the low-roughness microfacet
case SURVEY.md section 7's rule (error against the fp64 reference <= max(1e-4, 2 x the fp32 reference's own error))."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import assert_close, elementwise_rel_err, load_golden, rel_err, report_worst

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_objects_spec", os.path.join(os.path.dirname(__file__), "test_objects_cpu.py"))
spec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spec)

CENTRE, RADIUS, EYE = np.array([0.5, -0.1, 0.8]), 0.35, (0.02, 0.01, -0.03)


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


def make_model(cls, mode, **kw):
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    extra = dict(mlp_num_density_channels=5, num_env_samples=10) if cls == "pano" else {}
    model = (pn.PanoMipNeRF if cls == "pano" else pn.MipNeRF)(num_samples=16, rgb_activation="softplus", **extra, **kw)
    model.mlp.load_state_dict(orc.init_params(4, 5 if cls == "pano" else 1))
    model = model.to(dev())
    model.mlp_mode = mode
    return model


def probe_tensor(pix, H, W, contiguous=False):
    """[K, HW, 3] host radiance -> [K, 3, H, W] device tensor: the strided view of a [K, H, W, 3] buffer that light_probes
    returns, or a contiguous copy."""
    x = T(pix).view(-1, H, W, 3).permute(0, 3, 1, 2)
    return x.contiguous() if contiguous else x


# ----------------------------------------------------------------------------------------------------- 1. shade
def _golden_case(size):
    g = load_golden("objects_ref")
    H, W = (int(s) for s in size.split("x"))
    k = size + "/"
    return g, k, H, W, probe_tensor(g[k + "probes"], H, W), T(g[k + "albedo"]), T(g[k + "normal"]), T(-g[k + "v"])


@pytest.mark.parametrize("size", ["16x32", "32x64"])
def test_shade_matches_the_reference(size):
    from pano_nerf_amd import objects
    g, k, H, W, probes, a, n, vd = _golden_case(size)
    names = ("rgb", "diffuse", "specular", "shading")
    got = objects.shade(probes[:1], a, n, vd)
    for name, x in zip(names, got):
        assert_close(N(x), g[k + "lambert/" + name], f"objects/{size}/lambert/{name}")
    got = objects.shade(probes, a, n, vd, None, T(g[k + "weights"]))
    for name, x in zip(names, got):
        assert_close(N(x), g[k + "lambert_k3/" + name], f"objects/{size}/lambert_k3/{name}")
    got = objects.shade(probes[:1], a, n, vd, T(g[k + "micro_hi/roughness"]))
    assert got[3] is None
    for name, x in zip(names[:3], got):
        assert_close(N(x), g[k + "micro_hi/" + name], f"objects/{size}/micro_hi/{name}")


@pytest.mark.parametrize("size", ["16x32", "32x64"])
def test_shade_low_roughness_against_the_fp64_reference(size):
    """The fp32 reference is itself ~7e-4 off its fp64 run here (cancellation in NoH^2 (alpha^2 - 1) + 1): SURVEY section 7."""
    from pano_nerf_amd import objects
    g, k, H, W, probes, a, n, vd = _golden_case(size)
    got = objects.shade(probes[:1], a, n, vd, T(g[k + "micro_lo/roughness"]))
    for name, x in zip(("rgb", "diffuse", "specular"), got):
        r32, r64 = g[k + f"micro_lo/{name}"], g[k + f"micro_lo/{name}64"]
        ours, theirs = rel_err(N(x), r64), rel_err(r32, r64)
        ours_e, theirs_e = elementwise_rel_err(N(x), r64), elementwise_rel_err(r32, r64)
        print(size, name, "tensor-scale ours / fp32 reference:", ours, theirs, "element-wise:", ours_e, theirs_e)
        report_worst(f"objects micro_lo {name}: ours vs fp64 (tensor-scale)", ours)
        report_worst(f"objects micro_lo {name}: fp32 reference vs fp64 (tensor-scale)", theirs)
        report_worst(f"objects micro_lo {name}: ours vs fp64 (element-wise)", ours_e)
        report_worst(f"objects micro_lo {name}: fp32 reference vs fp64 (element-wise)", theirs_e)
        assert ours <= max(1e-4, 2 * theirs), (name, ours, theirs)
        assert ours_e <= max(1e-4, 2 * theirs_e), (name, ours_e, theirs_e)


def test_shade_layouts_roughness_forms_edge_rows_and_blends():
    from pano_nerf_amd import lighting, objects
    g, k, H, W, probes, a, n, vd = _golden_case("16x32")
    rough = T(g[k + "micro_hi/roughness"])
    w = T(g[k + "weights"])
    # strided [K, H, W, 3]-backed probes and contiguous ones: the same bits
    assert not probes.is_contiguous()
    for args in ((None, w), (rough, w)):
        x, y = objects.shade(probes, a, n, vd, *args), objects.shade(probes.contiguous(), a, n, vd, *args)
        assert all(bits_equal(p, q) for p, q in zip(x[:3], y[:3]))
    # a float roughness is the [R, 1] tensor of it
    x = objects.shade(probes[:1], a, n, vd, 0.45)
    y = objects.shade(probes[:1], a, n, vd, torch.full((a.shape[0], 1), 0.45, device=dev()))
    assert all(bits_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] is None
    # against the fp64 restatement on a row count that is no multiple of the workgroup
    dirs, omega = lighting.probe_directions(H, W, dev())
    R = 201
    for args in ((None, None), (rough[:R], None)):
        got = objects.shade(probes[:1], a[:R], n[:R], vd[:R], *args)
        want = spec.shade(g[k + "probes"][:1], N(dirs), N(omega), N(a[:R]), N(n[:R]), N(vd[:R]),
                          None if args[0] is None else N(args[0]))
        for p, q in zip(got[:3], want[:3]):
            assert rel_err(N(p), q) < 1e-6 or not np.abs(q).max()
    # NoV == 0 (grazing view), a view from behind and a zero normal (NoL == 0 everywhere): finite, the reference's NaN -> 0
    n2 = T([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    v2 = T([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    for r in (0.05, 0.5, 1.0):
        rgb, diffuse, specular, _ = objects.shade(probes[:1], a[:3], n2, v2, r)
        assert bool(torch.isfinite(rgb).all()) and bool((specular == 0).all()) and bool((diffuse[2] == 0).all())
        assert bool((diffuse[:2] > 0).all())
    # K = 3 microfacet with the same weights on every row = K = 1 on the probe blended in fp64 and rounded once
    wrow = np.array([0.5, 0.3, 0.2], np.float32)
    blend = np.einsum("k,kpc->pc", wrow.astype(np.float64), g[k + "probes"].astype(np.float64)).astype(np.float32)
    x = objects.shade(probes, a, n, vd, rough, T(np.tile(wrow, (a.shape[0], 1))))
    y = objects.shade(probe_tensor(blend[None], H, W), a, n, vd, rough)
    for p, q in zip(x[:3], y[:3]):
        assert rel_err(N(p), N(q)) < 1e-6


# ------------------------------------------------------------------------------------------------- 2. trace_mesh
def _ray_sets():
    return dict(pano=spec.pano_rays(128, 256, EYE), pinhole=spec.pinhole_rays(96, 128, 60.0, spec.look_at(EYE, CENTRE)))


@pytest.mark.parametrize("kind", ["pano", "pinhole"])
def test_trace_mesh_matches_the_fp64_restatement(kind):
    from pano_nerf_amd import objects
    v, f = spec.icosphere(3, RADIUS, CENTRE)
    assert f.shape[0] == 1280
    o, d = (x.astype(np.float32) for x in _ray_sets()[kind])
    to, td, tv, tf = T(o), T(d), T(v), T(f, torch.int32)
    t, face, bary = objects.trace_mesh(to, td, tv, tf)
    assert t.dtype == torch.float32 and face.dtype == torch.int32 and bary.shape == (o.shape[0], 2)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    rt, rface, rbary, near = spec.trace(o64, d64, v, f, margin=1e-4)
    dist, tc = spec.line_distance(o64, d64, CENTRE)
    reach = (dist <= 1.05 * RADIUS) & (tc > 0)
    share = float((near & reach).sum()) / float(reach.sum())
    print(kind, "rays reaching the bounding sphere x 1.05:", int(reach.sum()), "hits:", int(np.isfinite(rt).sum()),
          "left out:", int((near & reach).sum()), "share:", share)
    assert share <= 0.03, share
    keep = ~near
    gt, gface, gbary = N(t), N(face), N(bary)
    assert np.array_equal(np.isfinite(gt)[keep], np.isfinite(rt)[keep])
    assert np.array_equal(gface[keep], rface[keep])
    hit = keep & (rface >= 0)
    e_t = float(np.max(np.abs(gt[hit] - rt[hit]) / rt[hit]))
    e_b = float(np.max(np.abs(gbary[hit] - rbary[hit])))
    report_worst(f"objects trace {kind}: t relative", e_t)
    report_worst(f"objects trace {kind}: barycentrics absolute", e_b)
    assert e_t <= 1e-4 and e_b <= 1e-4, (e_t, e_b)
    assert np.all(np.isinf(gt[gface < 0])) and np.all(gbary[gface < 0] == 0)
    # no leaks: every ray whose line passes within 0.99 x the inscribed radius of the centre hits (margin rays included)
    vt = v.astype(np.float64)
    nrm = np.cross(vt[f[:, 1]] - vt[f[:, 0]], vt[f[:, 2]] - vt[f[:, 0]])
    r_in = float((((vt[f[:, 0]] - CENTRE) * nrm).sum(1) / np.linalg.norm(nrm, axis=1)).min())
    inner = (dist < 0.99 * r_in) & (tc > 0)
    assert inner.sum() > 500 and np.isfinite(gt[inner]).all()
    # t_max: exclusive, per ray
    tm = np.where(np.arange(len(gt)) % 2 == 0, gt * 0.5, gt * 2.0).astype(np.float32)
    tm[~np.isfinite(tm)] = 1.0
    t2, face2, _ = objects.trace_mesh(to, td, tv, tf, t_max=T(tm))
    far_side = N(t2) < tm  # a ray cut short of its first hit may still see nothing, never something beyond t_max
    assert np.all(far_side[N(face2) >= 0])
    odd = (np.arange(len(gt)) % 2 == 1) & (gface >= 0)
    assert np.array_equal(N(face2)[odd], gface[odd]) and np.array_equal(N(t2)[odd], gt[odd])
    even = (np.arange(len(gt)) % 2 == 0) & (gface >= 0)
    assert np.all(N(face2)[even] < 0)
    t3, _, _ = objects.trace_mesh(to, td, tv, tf, t_max=t)  # t < t_max with t_max = t: nothing closer
    assert bool(torch.isinf(t3).all())
    # any_hit
    any_hit = objects.trace_mesh(to, td, tv, tf, any_hit=True)
    assert any_hit.dtype == torch.bool and np.array_equal(N(any_hit), np.isfinite(gt))
    # the number of rays per launch does not show
    for R in (1, 63, 64, 65, 4097):
        a, b, c = objects.trace_mesh(to[:R], td[:R], tv, tf)
        assert bits_equal(a, t[:R]) and bits_equal(b, face[:R]) and bits_equal(c, bary[:R]), R
    first = int(np.nonzero(gface >= 0)[0][0])  # a window that holds hits, at an offset that is no multiple of 64
    sl = slice(max(first - 7, 0), max(first - 7, 0) + 4097)
    a, b, c = objects.trace_mesh(to[sl], td[sl], tv, tf)
    assert bits_equal(a, t[sl]) and bits_equal(b, face[sl]) and bits_equal(c, bary[sl])
    # the order of the faces does not show, except in exact ties
    perm = np.random.default_rng(3).permutation(f.shape[0])
    tp, fp, bp = objects.trace_mesh(to, td, tv, T(f[perm], torch.int32))
    assert bits_equal(tp, t)
    mapped = np.where(N(fp) >= 0, perm[np.maximum(N(fp), 0)], -1)
    same = mapped == gface
    assert (~same).sum() <= 0.01 * max(1, (gface >= 0).sum()), (~same).sum()  # ties: the closest t is the same, bit for bit
    assert np.array_equal(N(bp)[same], gbary[same])
    # F = 0: all misses; R = 0: empty outputs
    t0, f0, b0 = objects.trace_mesh(to, td, tv, tf[:0])
    assert bool(torch.isinf(t0).all()) and bool((f0 == -1).all()) and bool((b0 == 0).all())
    assert not bool(objects.trace_mesh(to, td, tv, tf[:0], any_hit=True).any())
    assert objects.trace_mesh(to[:0], td[:0], tv, tf)[0].shape == (0,)
    # a face that points outside the vertices is never hit (and never read)
    bad = f.copy()
    bad[::2, 1] = v.shape[0] + 5
    tb, fb, _ = objects.trace_mesh(to, td, tv, T(bad, torch.int32))
    assert not np.any(N(fb)[N(fb) >= 0] % 2 == 0)


@pytest.mark.parametrize("kind", ["pano", "pinhole"])
def test_trace_mesh_is_the_fp32_restatement_bit_for_bit(kind):
    """The kernel's arithmetic is separate fp32 operations in the header's order (no contraction, a correctly rounded
    1 / det), so numpy evaluates the same numbers: every ray, the ones near an edge included."""
    from pano_nerf_amd import objects
    v, f = spec.icosphere(3, RADIUS, CENTRE)
    o, d = (x.astype(np.float32) for x in _ray_sets()[kind])
    t, face, bary = objects.trace_mesh(T(o), T(d), T(v), T(f, torch.int32))
    rt, rface, rbary = spec.trace(o, d, v, f, dtype=np.float32)
    assert rt.dtype == np.float32 and rbary.dtype == np.float32
    assert np.array_equal(N(face), rface)
    assert np.array_equal(N(t).view(np.int32), rt.view(np.int32))
    assert np.array_equal(N(bary).view(np.int32), rbary.view(np.int32))


# ----------------------------------------------------------------------------------------------- 3. shadow_ratio
def _hdr_probe(H, W):
    rng = np.random.Generator(np.random.PCG64(7))
    env = rng.random((H * W, 3)) * 2.0
    env[rng.random(H * W) < 0.02] *= 25.0
    return env.astype(np.float32)


def _floor(G, y=-0.5):
    X, Z = np.meshgrid(np.linspace(-0.5, 1.5, G), np.linspace(-0.2, 1.8, G), indexing="ij")
    pts = np.stack([X, np.full_like(X, y), Z], -1).reshape(-1, 3).astype(np.float32)
    return pts, np.tile(np.array([[0, 1, 0]], np.float32), (len(pts), 1))


@pytest.mark.parametrize("H,W,G", [(8, 16, 64), (16, 32, 48)])
def test_shadow_ratio_matches_the_fp64_restatement(H, W, G):
    from pano_nerf_amd import lighting, objects
    v, f = spec.icosphere(3, RADIUS, CENTRE)
    env = _hdr_probe(H, W)
    pts, nrm = _floor(G)
    probe = probe_tensor(env[None], H, W)[0]
    tv, tf = T(v), T(f, torch.int32)
    got = objects.shadow_ratio(T(pts), T(nrm), probe, tv, tf, bias=1e-3)
    assert got.shape == (G * G,) and got.dtype == torch.float32
    dirs, omega = lighting.probe_directions(H, W, dev())
    want, share, pairs = spec.shadow_ratio(pts, nrm, env, N(dirs), N(omega), v, f, bias=1e-3, margin=1e-5)
    compared = share < 1e-3
    left = 1.0 - float(compared.mean())
    err = float(np.abs(N(got) - want)[compared].max())
    print(f"{H}x{W}: candidate pairs {pairs}, points not compared {left:.4f}, worst |ratio error| {err:.2e}, "
          f"ratios {N(got).min():.3f} .. {N(got).max():.6f}")
    report_worst(f"objects shadow {H}x{W}: ratio absolute", err)
    assert left <= 0.05, left
    assert err <= 1e-5, err
    g = N(got)
    assert g.min() >= 0.0 and g.max() <= 1.0 and g.min() < 0.5 and g.max() < 1.0  # every floor point sees the sphere
    # exactly 1 above the sphere (it is below the horizon of an upward normal) and without faces
    up, _ = _floor(G, 0.6)
    assert bool((objects.shadow_ratio(T(up), T(nrm), probe, tv, tf) == 1.0).all())
    assert bool((objects.shadow_ratio(T(pts), T(nrm), probe, tv, tf[:0]) == 1.0).all())
    # non-finite points -> 1, their neighbours untouched
    p2 = pts.copy()
    p2[5, 0], p2[77, 1], p2[300, 2] = np.nan, np.inf, -np.inf
    g2 = N(objects.shadow_ratio(T(p2), T(nrm), probe, tv, tf))
    idx = np.array([5, 77, 300])
    assert np.all(g2[idx] == 1.0) and np.array_equal(np.delete(g2, idx), np.delete(g, idx))
    assert objects.shadow_ratio(T(pts[:0]), T(nrm[:0]), probe, tv, tf).shape == (0,)
    if (H, W) == (8, 16):  # the number of points per launch does not show
        tp, tn = T(pts), T(nrm)
        for R in (1, 65, 4096):
            assert bits_equal(objects.shadow_ratio(tp[:R], tn[:R], probe, tv, tf), got[:R]), R
        assert bits_equal(objects.shadow_ratio(tp[1000:1065], tn[1000:1065], probe, tv, tf), got[1000:1065])
        assert bits_equal(objects.shadow_ratio(tp, tn, probe.contiguous()[None], tv, tf), got)


# ---------------------------------------------------------------------------------------------- 4. insert_object
def _cameras():
    from pano_nerf_amd import views
    return dict(pano=views.pano_camera(32, 64), pinhole=views.perspective_camera(24, 32, fov_x_deg=60.0))


def _object(level=2, radius=0.2, centre=(0.0, 0.0, -0.6), **kw):
    from pano_nerf_amd import objects
    v, f = spec.icosphere(level, radius, centre)
    return objects.VirtualObject(T(v), T(f, torch.int32), **kw)


def _by_hand(model, camera, c2w, obj, probe_positions=None, probe_size=(16, 32), shadows=True, shadow_probe=(8, 16),
             bias=1e-3):
    """insert_object composed from the public pieces."""
    import pano_nerf_amd as pn
    from pano_nerf_amd import lighting, objects, views
    H, W = camera.h, camera.w
    scene = views.render_view(model, camera, c2w, outputs=("rgb", "depth", "normal"))
    rows = lambda x: x.permute(0, 2, 3, 1).reshape(H * W, -1)
    s_rgb, s_dep, s_nor = rows(scene["fine_rgb"]), rows(scene["fine_dep"]), rows(scene["fine_nor"])
    pos = obj.centroid() if probe_positions is None else probe_positions
    probes = lighting.light_probes(model, pos, *probe_size)
    rays = pn.generate_pano_rays(H, W, c2w) if isinstance(camera, views.PanoCamera) else \
        views.generate_perspective_rays(camera, c2w)
    t, face, bary = objects.trace_mesh(rays.origins, rays.directions, obj.vertices, obj.faces)
    K = pos.shape[0]
    at = objects.hit_attributes(obj, rays.origins, rays.directions, t, face, bary, s_dep, pos if K > 1 else None)
    m = at["mask"]
    object_rgb = torch.zeros(H * W, 3, device=dev())
    if bool(m.any()):
        object_rgb[m] = objects.shade(probes, at["albedo"][m], at["normals"][m], at["viewdirs"][m], obj.roughness,
                                      at["weights"][m] if K > 1 else None)[0]
    if shadows:
        sprobe = lighting.light_probes(model, obj.centroid(), *shadow_probe)
        shadow = objects.shadow_ratio(at["scene_points"], s_nor, sprobe, obj.vertices, obj.faces, bias)
    else:
        shadow = torch.ones(H * W, device=dev())
    rgb = torch.where(m[:, None], object_rgb, s_rgb * shadow[:, None])
    depth = torch.where(m, t, s_dep[:, 0])
    img = lambda x: x.reshape(1, H, W, -1).permute(0, 3, 1, 2)
    return dict(scene_rgb=scene["fine_rgb"], scene_dep=scene["fine_dep"], scene_nor=scene["fine_nor"],
                mask=img(m.float()), object_rgb=img(object_rgb), shadow=img(shadow), rgb=img(rgb), depth=img(depth)), at, t


C2W = spec.look_at((0.1, 0.05, 0.2), (0.0, 0.0, -0.6))


@pytest.mark.parametrize("mode", ["fused_f16x2", "layerwise"])
@pytest.mark.parametrize("cam", ["pano", "pinhole"])
def test_insert_object_is_the_composition_of_its_pieces(mode, cam):
    from pano_nerf_amd import objects
    model = make_model("pano", mode)
    camera = _cameras()[cam]
    obj = _object(roughness=0.4 if cam == "pinhole" else None)
    out = objects.insert_object(model, camera, C2W, obj, probe_size=(16, 32))
    want, at, t = _by_hand(model, camera, C2W, obj)
    assert set(out) == set(want)
    for k in want:
        assert out[k].shape == want[k].shape and out[k].dtype == torch.float32, k
        assert bits_equal(out[k], want[k]), (mode, cam, k)
    m = out["mask"][0, 0] > 0
    print(mode, cam, "masked pixels:", int(m.sum()), "of", m.numel(), "shadow min:", float(out["shadow"].min()),
          "scene depth:", float(out["scene_dep"].min()), "..", float(out["scene_dep"].max()))
    assert bool(torch.isfinite(out["object_rgb"]).all()) and bool((out["object_rgb"][0, :, ~m] == 0).all())
    assert bool((out["shadow"][0, 0][m] == 1).all()) and float(out["shadow"].min()) >= 0 and float(out["shadow"].max()) <= 1
    # chunk_rays is invisible
    out2 = objects.insert_object(model, camera, C2W, obj, probe_size=(16, 32), chunk_rays=camera.h * camera.w // 4 + 3)
    assert all(bits_equal(out[k], out2[k]) for k in out)
    # shadows=False
    out3 = objects.insert_object(model, camera, C2W, obj, probe_size=(16, 32), shadows=False)
    assert bool((out3["shadow"] == 1).all()) and bits_equal(out3["mask"], out["mask"])
    assert bits_equal(out3["rgb"], torch.where(m[None, None], out["object_rgb"], out["scene_rgb"]))


def test_insert_object_occlusion_by_the_scene():
    from pano_nerf_amd import objects
    model = make_model("pano", "fused_f16x2")
    camera = _cameras()["pinhole"]
    eye = C2W[:3, 3]
    ahead = -C2W[:3, 2]
    # beyond far: hidden wherever the scene's depth is finite
    obj = _object(centre=tuple(eye + 12.0 * ahead), radius=2.0)
    out = objects.insert_object(model, camera, C2W, obj, probe_size=(8, 16))
    finite = torch.isfinite(out["scene_dep"][0, 0])
    assert bool(finite.any())
    assert bool((out["mask"][0, 0][finite] == 0).all())
    want = out["scene_rgb"] * out["shadow"]
    assert bits_equal(out["rgb"][0][:, finite], want[0][:, finite])
    # in front of everything: the mask is the tracer's hit set
    obj = _object(centre=tuple(eye + 0.05 * ahead), radius=0.01)
    out = objects.insert_object(model, camera, C2W, obj, probe_size=(8, 16))
    from pano_nerf_amd import views
    rays = views.generate_perspective_rays(camera, C2W)
    t, face, _ = objects.trace_mesh(rays.origins, rays.directions, obj.vertices, obj.faces)
    assert bool((face >= 0).any())
    assert torch.equal(out["mask"].reshape(-1) > 0, face >= 0)
    assert bits_equal(out["depth"].reshape(-1)[face >= 0], t[face >= 0])


def test_insert_object_mipnerf_and_several_probes():
    from pano_nerf_amd import objects
    camera = _cameras()["pinhole"]
    obj = _object()
    out = objects.insert_object(make_model("mip", "fused_f16x2"), camera, C2W, obj, probe_size=(8, 16))
    assert bool(torch.isfinite(out["rgb"]).all()) and float(out["mask"].sum()) > 0
    model = make_model("pano", "fused_f16x2")
    one = objects.insert_object(model, camera, C2W, obj, probe_size=(8, 16))
    pos = T([[0.3, 0.2, -0.5], [-0.4, -0.1, -0.9]])
    two = objects.insert_object(model, camera, C2W, obj, probe_positions=pos, probe_size=(8, 16))
    want, at, _ = _by_hand(model, camera, C2W, obj, probe_positions=pos, probe_size=(8, 16))
    assert all(bits_equal(two[k], want[k]) for k in want)
    assert bits_equal(one["mask"], two["mask"]) and not bits_equal(one["object_rgb"], two["object_rgb"])
    m = at["mask"]
    w = N(at["weights"])
    assert w.shape == (camera.h * camera.w, 2) and np.allclose(w[N(m)].sum(1), 1.0, atol=1e-6) and np.all(w[~N(m)] == 0)
    assert np.all(w >= 0)


def test_hit_attributes_match_the_fp64_restatement():
    from pano_nerf_amd import objects
    v, f = spec.icosphere(2, RADIUS, CENTRE)
    o, d = (x.astype(np.float32) for x in spec.pinhole_rays(48, 64, 60.0, spec.look_at(EYE, CENTRE)))
    vn = ((v.astype(np.float64) - CENTRE) / RADIUS).astype(np.float32)
    col = np.random.default_rng(4).random(v.shape).astype(np.float32)
    dep = np.full(o.shape[0], 0.8, np.float32)
    dep[::7] = np.nan
    pos = np.array([[0.5, -0.1, 0.8], [0.2, 0.3, 0.4], [0.9, 0.0, 0.2]], np.float32)
    for normals, albedo in ((None, (0.2, 0.4, 0.6)), (vn, col)):
        obj = objects.VirtualObject(T(v), T(f, torch.int32), None if normals is None else T(normals),
                                    T(albedo) if isinstance(albedo, np.ndarray) else albedo)
        t, face, bary = objects.trace_mesh(T(o), T(d), obj.vertices, obj.faces)
        at = objects.hit_attributes(obj, T(o), T(d), t, face, bary, T(dep), T(pos))
        want = spec.hit_attributes(o, d, N(t), N(face), N(bary), v, f, normals, albedo, dep, pos)
        assert np.array_equal(N(at["mask"]), want["mask"]) and want["mask"].any() and (~want["mask"] & (N(face) >= 0)).any()
        for k in ("points", "normals", "albedo", "viewdirs", "weights"):
            assert np.abs(N(at[k]) - want[k]).max() <= 1e-6, k
        sp, wp = N(at["scene_points"]), want["scene_points"]
        assert np.array_equal(np.isnan(sp), np.isnan(wp)) and np.nanmax(np.abs(sp - wp)) <= 1e-6
    # without a scene depth every hit is in the mask
    at = objects.hit_attributes(obj, T(o), T(d), t, face, bary)
    assert torch.equal(at["mask"], face >= 0) and "scene_points" not in at and "weights" not in at
    # helpers
    moved = obj.transformed(np.array([[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]))
    assert np.allclose(N(moved.vertices), v + np.array([0.5, 0, 0], np.float32), atol=1e-6)
    assert np.allclose(N(moved.normals), vn, atol=1e-6)
    from pano_nerf_amd import geometry
    m = objects.VirtualObject.from_mesh(geometry.Mesh(v, f, vn, col), device=dev())
    assert bits_equal(m.vertex_albedo, T(col)) and bits_equal(m.normals, T(vn)) and m.faces.dtype == torch.int32


def test_insert_path_frames_and_files(tmp_path):
    from pano_nerf_amd import io_exr, objects, views
    model = make_model("pano", "fused_f16x2")
    camera = _cameras()["pinhole"]
    obj = _object()
    poses = np.stack([spec.look_at((0.1 + 0.05 * i, 0.05, 0.2), (0.0, 0.0, -0.6)) for i in range(3)])
    frames = objects.insert_path(model, camera, poses, obj, probe_size=(8, 16), kinds=("ldr", "mask"))
    assert set(frames) == {"ldr", "mask"}
    for k in frames:
        assert frames[k].shape == (3, camera.h, camera.w, 3) and frames[k].dtype == torch.uint8
    for i in range(3):
        out = objects.insert_object(model, camera, poses[i], obj, probe_size=(8, 16))
        assert torch.equal(frames["ldr"][i], views.to_frame(out["rgb"], "ldr"))
        assert torch.equal(frames["mask"][i][..., 0] > 0, out["mask"][0, 0] > 0)
    assert objects.insert_path(model, camera, poses, obj, probe_size=(8, 16), out_dir=str(tmp_path)) == {}
    for k in ("ldr", "mask"):
        assert sorted(os.listdir(tmp_path / k)) == [f"{i:05d}.png" for i in range(3)]
    if hasattr(io_exr, "read_png"):
        assert np.array_equal(io_exr.read_png(str(tmp_path / "ldr" / "00001.png")), N(frames["ldr"][1]))
    with pytest.raises(ValueError, match="kinds"):
        objects.insert_path(model, camera, poses, obj, kinds=("albedo",))


# -------------------------------------------------------------------------------------------- 5. argument errors
def test_argument_errors():
    from pano_nerf_amd import objects
    v, f = spec.icosphere(0)
    tv, tf = T(v), T(f, torch.int32)
    z = torch.zeros(4, 3, device=dev())
    probes = torch.rand(9, 3, 4, 8, device=dev())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objects.trace_mesh(z.cpu(), z, tv, tf)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objects.shade(probes[:1], z, z.cpu(), z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objects.shadow_ratio(z, z, probes[0].cpu(), tv, tf)
    with pytest.raises(ValueError, match="at most 8"):
        objects.shade(probes, z, z, z, None, torch.rand(4, 9, device=dev()))
    with pytest.raises(ValueError, match="need weights"):
        objects.shade(probes[:2], z, z, z)
    with pytest.raises(ValueError, match="weights must be"):
        objects.shade(probes[:2], z, z, z, None, torch.rand(4, 3, device=dev()))
    with pytest.raises(ValueError, match="normals has 3 rows"):
        objects.shade(probes[:1], z, z[:3], z)
    with pytest.raises(ValueError, match="roughness"):
        objects.shade(probes[:1], z, z, z, torch.rand(3, 1, device=dev()))
    with pytest.raises(ValueError, match="directions has"):
        objects.trace_mesh(z, z[:2], tv, tf)
    with pytest.raises(ValueError, match="t_max"):
        objects.trace_mesh(z, z, tv, tf, t_max=torch.ones(3, device=dev()))
    with pytest.raises(ValueError, match="faces must"):
        objects.trace_mesh(z, z, tv, tf.float())
    with pytest.raises(ValueError, match="faces must"):
        objects.trace_mesh(z, z, tv, tf[:, :2])
    with pytest.raises(ValueError, match="one probe"):
        objects.shadow_ratio(z, z, probes[:2], tv, tf)
    with pytest.raises(ValueError, match="outside the 12 vertices"):
        objects.VirtualObject(tv, tf + 1)
    with pytest.raises(ValueError, match=r"one colour or \[V, 3\]"):
        objects.VirtualObject(tv, tf, albedo=torch.rand(5, 3, device=dev()))
    with pytest.raises(ValueError, match=r"one colour or \[V, 3\]"):
        objects.VirtualObject(tv, tf, albedo=(0.5, 0.5))
    with pytest.raises(ValueError, match="normals must be"):
        objects.VirtualObject(tv, tf, normals=torch.rand(5, 3, device=dev()))
    obj = objects.VirtualObject(v, f, device=dev())  # host arrays are copied to the device
    assert obj.vertices.device.type == "cuda" and obj.albedo == (0.8, 0.8, 0.8)
    model = make_model("pano", "fused_f16x2")
    cam = _cameras()["pinhole"]
    with pytest.raises(ValueError, match="VirtualObject"):
        objects.insert_object(model, cam, C2W, (tv, tf))
    with pytest.raises(ValueError, match="probe_positions"):
        objects.insert_object(model, cam, C2W, obj, probe_positions=torch.zeros(9, 3, device=dev()))
    with pytest.raises(ValueError, match="camera must come from"):
        objects.insert_object(model, (24, 32), C2W, obj)
    with pytest.raises(ValueError, match="chunk_rays"):
        objects.insert_object(model, cam, C2W, obj, chunk_rays=0)
