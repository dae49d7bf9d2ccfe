"""Texture-mapped materials on the GPU: ingest and the mip pyramid bit for bit against numpy, the sampler against the fp64
restatement of tests/_textures_ref.py on hits handed in directly (no tracer), the fall-backs of the normal map,
insert_object of a textured quad against the composition of its public pieces, and argument errors.

Tolerances (from the number formats, not from the kernels): sampled values lie in [0, 1] and both sides evaluate in fp64 and
round once to fp32, so they differ by at most one fp32 rounding at 1.0 = 2^-23, doubled for the fp64 noise that can move
a value across a rounding boundary: 2^-22.  The level of detail is rounded once from fp64 too: one fp32 ulp of the value."""
import functools

import numpy as np
import pytest
import torch

import _textures_ref as ref

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -22


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


# ------------------------------------------------------------------------------------------ 1. ingest and pyramid
@pytest.mark.parametrize("size", [(1, 1), (2, 2), (5, 3), (3, 8), (64, 64)])
def test_ingest_and_pyramid_bit_for_bit(size):
    from pano_nerf_amd import objects
    H, W = size
    rng = np.random.default_rng(H * 100 + W)
    u8 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    u8[0, 0] = (0, 255, 10)  # both ends of the table and the linear toe of the sRGB curve
    cases = [(u8, True), (u8, False), (rng.random((H, W, 3)).astype(np.float32) * 4.0 - 1.0, False),
             (rng.integers(0, 256, (H, W, 4), dtype=np.uint8), True), (rng.integers(0, 256, (H, W), dtype=np.uint8), False),
             (rng.random((H, W, 1)).astype(np.float32), False)]
    for img, srgb in cases:
        tex = objects.Texture(img, srgb=srgb, device=dev())
        levels = ref.pyramid(ref.level0(img, srgb))
        shapes = ref.level_shapes(H, W)
        assert (tex.H, tex.W, tex.L) == (H, W, len(levels)) and tex.C == (1 if img.ndim == 2 else img.shape[2])
        assert tuple(tex.data.shape) == (shapes[-1][0] + shapes[-1][1] * shapes[-1][2], 4) and tex.data.dtype == torch.float32
        assert torch.equal(tex.data.cpu().view(torch.int32), torch.from_numpy(ref.flat_pyramid(levels)).view(torch.int32))
        for l, (off, h, w) in enumerate(shapes):
            assert tex.level_shape(l) == (off, h, w)
            got = tex.level(l)
            assert tuple(got.shape) == (h, w, 4) and got.data_ptr() == tex.data.data_ptr() + off * 16
            assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(levels[l]).view(torch.int32)), (size, srgb, l)
    # a device tensor is taken as it is
    t2 = objects.Texture(T(u8, torch.uint8), srgb=True)
    assert bits_equal(t2.data, objects.Texture(u8, srgb=True, device=dev()).data)


# -------------------------------------------------------------------------------------------------- 2. the sampler
R_ROWS = 257
SIZES = dict(a=((16, 16), (5, 3), (16, 16)), b=((5, 3), (16, 16), (5, 3)))  # albedo, roughness, normal


@functools.lru_cache(maxsize=None)
def scene():
    """A small mesh with per-corner UVs (outside [0, 1] on both sides), a face whose UV triangle is degenerate (5) and one
    that reads a non-finite UV (6); textures of random values in [0, 1]; 257 hits handed in directly."""
    rng = np.random.default_rng(7)
    v = np.array([[0, 0, 0], [1, 0, 0.1], [1, 1, 0], [0, 1, -0.1], [0.5, 0.5, 0.8], [1.7, 0.2, 0.5], [-0.6, 0.4, 0.3]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 5], [3, 0, 6], [2, 3, 4], [1, 5, 4]], np.int32)
    uv = (rng.random((14, 2)) * 4.0 - 1.5).astype(np.float32)
    fuv = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [0, 0, 0], [1, 13, 2]], np.int32)
    uv[4:7] = [[-1.25, 0.5], [-0.5, 2.25], [0.75, -1.0]]  # well outside [0, 1] on both sides
    uv[13] = [np.inf, 0.25]
    fuv[5] = [3, 3, 7]  # two corners share a UV: det == 0
    F = len(f)
    face = rng.integers(0, F, R_ROWS).astype(np.int32)
    face[:7] = np.arange(7)
    a, b = rng.random(R_ROWS), rng.random(R_ROWS)
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    bary = np.stack([a, b], 1).astype(np.float32)
    bary[7], bary[8], bary[9] = (0, 0), (1, 0), (0, 1)  # the corners
    p = v.astype(np.float64)
    e1, e2 = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
    g = np.cross(e1, e2)
    A_w = np.linalg.norm(g, axis=1)
    ng = g / A_w[:, None]
    q = uv.astype(np.float64)
    with np.errstate(all="ignore"):
        d1, d2 = q[fuv[:, 1]] - q[fuv[:, 0]], q[fuv[:, 2]] - q[fuv[:, 0]]
        A_uv = np.abs(d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1])
    # directions: not normalised, never grazing (|n_g . d| / |d| >= 0.05 by construction: at least 0.25 here)
    d = np.empty((R_ROWS, 3), np.float32)
    nrm = np.empty((R_ROWS, 3), np.float32)
    for r in range(R_ROWS):
        n = ng[face[r]]
        while True:
            x = rng.normal(size=3)
            x /= np.linalg.norm(x)
            if abs(x @ n) >= 0.25:
                break
        x = (x * rng.uniform(0.5, 3.0)).astype(np.float32)
        d[r] = x
        s = n if n @ x < 0 else -n  # towards the eye, then tilted like an interpolated normal
        s = s + 0.05 * rng.normal(size=3)
        nrm[r] = (s / np.linalg.norm(s)).astype(np.float32)
    assert np.all(np.abs(np.einsum("rc,rc->r", ng[face], d.astype(np.float64))) / np.linalg.norm(d.astype(np.float64), axis=1) >= 0.05)
    t = rng.uniform(0.5, 3.0, R_ROWS).astype(np.float32)
    mask = rng.random(R_ROWS) < 0.85
    mask[:10] = True
    mask[10] = False
    face[11], mask[11] = -1, False  # a miss
    textures = {}
    for key, sizes in SIZES.items():
        textures[key] = [rng.random((h, w, 3)).astype(np.float32) for h, w in sizes]
    # radii: aimed at levels of detail of the first (rows 0 mod 2) or the second (rows 1 mod 2) texture of set "a"
    c = np.abs(np.einsum("rc,rc->r", ng[face], d.astype(np.float64))) / np.linalg.norm(d.astype(np.float64), axis=1)
    radii = np.empty(R_ROWS, np.float32)
    targets = {}
    for k, (H, W) in enumerate(SIZES["a"][:2]):
        L = ref.num_levels(H, W)
        tg = [-2.0, L + 1.0] + [l + 0.5 for l in range(L - 1)] + [l + 0.25 for l in range(L - 1)]
        tg += [l + s * 5e-7 for l in range(1, L - 1) for s in (-1, 1)] + [float(l) for l in range(L)]
        targets[k] = tg
    for r in range(R_ROWS):
        k = r % 2
        H, W = SIZES["a"][k]
        tg = targets[k][(r // 2) % len(targets[k])]
        with np.errstate(all="ignore"):
            base = 0.5 * np.log2(W * H * A_uv[face[r]] / A_w[face[r]])
        width = 2.0 ** (tg - base + np.log2(c[r])) if np.isfinite(base) else 0.05
        radii[r] = np.float32(width / (2.0 * float(t[r])))
    return dict(v=v, f=f, uv=uv, fuv=fuv, face=face, bary=bary, d=d, t=t, normals=nrm, mask=mask, radii=radii,
                textures=textures)


@functools.lru_cache(maxsize=None)
def reference(key, wrap, flip_v, with_radii, rows):
    s = scene()
    tex = {n: ref.pyramid(ref.level0(img)) for n, img in zip(("albedo", "roughness", "normal"), s["textures"][key])}
    sl = slice(0, rows)
    return ref.texture_hits(s["mask"][sl], s["face"][sl], s["bary"][sl], s["d"][sl], s["t"][sl], s["normals"][sl],
                            s["radii"][sl] if with_radii else None, s["v"], s["f"], s["uv"], s["fuv"], tex, wrap, flip_v)


def textured_object(key, wrap, flip_v):
    from pano_nerf_amd import objects
    s = scene()
    maps = [objects.Texture(img, device=dev()) for img in s["textures"][key]]
    return objects.VirtualObject(s["v"], s["f"], roughness=0.5, device=dev(), uv=s["uv"], face_uv=s["fuv"],
                                 albedo_map=maps[0], roughness_map=maps[1], normal_map=maps[2], wrap=wrap, flip_v=flip_v)


def run_sampler(key, wrap, flip_v, with_radii, rows, bad_index=False):
    from pano_nerf_amd import objects
    s = scene()
    obj = textured_object(key, wrap, flip_v)
    if bad_index:  # the constructor refuses an index outside uv, so it goes in behind its back
        obj.face_uv = torch.where(obj.face_uv == 13, 99, obj.face_uv).contiguous()
    sl = slice(0, rows)
    return objects.sample_textures(obj, T(s["mask"][sl], torch.bool), T(s["face"][sl], torch.int32), T(s["bary"][sl]),
                                   T(s["d"][sl]), T(s["t"][sl]), T(s["normals"][sl]), T(s["radii"][sl]) if with_radii else None)


def check(got, want, mask, tag):
    ulp = np.spacing(np.abs(want["lod"]).astype(np.float32)).astype(np.float64)
    errs = {}
    for k in ("albedo", "roughness", "normals"):
        g = N(got[k]).astype(np.float64).reshape(want[k].shape)
        errs[k] = float(np.abs(g - want[k]).max())
        assert np.all(g[~mask] == 0), (tag, k)
    lod_err = np.abs(N(got["lod"]).astype(np.float64) - want["lod"].astype(np.float32).astype(np.float64))
    print(tag, "max abs error:", errs, "lod error in ulp:", float((lod_err / ulp).max()))
    for k, e in errs.items():
        assert e <= TOL, (tag, k, e)
    assert np.all(lod_err <= ulp), (tag, float((lod_err / ulp).max()))
    assert np.all(N(got["lod"])[~mask] == 0), tag


@pytest.mark.parametrize("flip_v", [True, False])
@pytest.mark.parametrize("wrap", ["repeat", "clamp"])
@pytest.mark.parametrize("key", ["a", "b"])
def test_sampler_matches_the_fp64_reference(key, wrap, flip_v):
    s = scene()
    want = reference(key, wrap, flip_v, True, R_ROWS)
    got = run_sampler(key, wrap, flip_v, True, R_ROWS)
    check(got, want, s["mask"], f"{key}/{wrap}/flip={flip_v}")
    m = s["mask"]
    if key == "a":
        # the levels of detail the radii were aimed at were reached: below 0 and above the top (clamped), inside every
        # interval, on the integers and within 1e-6 of them on either side
        for k, (H, W) in enumerate(SIZES["a"][:2]):
            lam = want["lod"][m & (np.arange(R_ROWS) % 2 == k) & ~np.isin(s["face"], (5, 6)), k]
            L = ref.num_levels(H, W)
            frac = lam - np.floor(lam)
            assert (lam == 0).any() and (lam == L - 1).any()
            for l in range(L - 1):
                assert ((lam > l + 0.1) & (lam < l + 0.9)).any(), (k, l)
            if L > 2:
                assert ((frac > 0) & (frac < 1e-6)).any() and ((frac > 1 - 1e-6) & (frac < 1)).any(), k
    # the degenerate face reads level 0 and keeps N; the non-finite UV samples 0 and keeps N
    deg, nonfin = m & (s["face"] == 5), m & (s["face"] == 6)
    assert deg.any() and nonfin.any()
    assert np.all(N(got["lod"])[deg] == 0)
    assert bits_equal(got["normals"][T(deg | nonfin, torch.bool)], T(s["normals"])[T(deg | nonfin, torch.bool)])
    assert np.all(N(got["albedo"])[nonfin] == 0) and np.all(N(got["roughness"])[nonfin] == 0)
    assert np.any(N(got["albedo"])[deg] != 0)
    # both outcomes of the normal map occur among the ordinary rows
    fb = want["fallback"][m & ~deg & ~nonfin]
    assert fb.any() and (~fb).any()


def test_sampler_one_row_no_radii_and_launch_size():
    s = scene()
    for rows in (1, R_ROWS):
        want = reference("a", "repeat", True, False, rows)
        got = run_sampler("a", "repeat", True, False, rows)
        check(got, want, s["mask"][:rows], f"no radii / {rows} rows")
        assert np.all(N(got["lod"]) == 0)
    one = run_sampler("a", "repeat", True, True, 1)
    check(one, reference("a", "repeat", True, True, 1), s["mask"][:1], "1 row")
    # the rows do not depend on the launch they are in
    full = run_sampler("a", "repeat", True, True, R_ROWS)
    part = run_sampler("a", "repeat", True, True, 200)
    assert all(bits_equal(full[k][:200], part[k]) for k in full)
    assert all(bits_equal(full[k][:1], one[k]) for k in full)
    # a face_uv index outside [0, T) reads as a non-finite (NaN) UV: the rows of face 6 give what its infinite UV gives -
    # samples 0, N kept - at level 0 (NaN -> 0; the infinite UV has an infinite A_uv and with it the top level)
    bad = run_sampler("a", "repeat", True, True, R_ROWS, bad_index=True)
    assert all(bits_equal(full[k], bad[k]) for k in ("albedo", "roughness", "normals"))
    six = T(s["face"] == 6, torch.bool)
    assert bits_equal(full["lod"][~six], bad["lod"][~six]) and bool((bad["lod"][six] == 0).all())
    assert bool((bad["albedo"][six] == 0).all()) and bits_equal(
        bad["normals"][six], torch.where(T(s["mask"], torch.bool)[:, None], T(s["normals"]), torch.zeros(1, device=dev()))[six])


# ------------------------------------------------------------------------------------------ 3. normal-map fall-backs
def test_normal_map_fallbacks():
    from pano_nerf_amd import objects
    s = scene()
    flat = np.tile(np.array([0.5, 0.5, 1.0], np.float32), (4, 4, 1))
    away = np.tile(np.array([0.5, 0.5, 0.0], np.float32), (4, 4, 1))  # m = (0, 0, -1): n = -N faces away from the eye
    keep = ~np.isin(s["face"], (5, 6)) & s["mask"]
    args = (T(s["mask"], torch.bool), T(s["face"], torch.int32), T(s["bary"]), T(s["d"]), T(s["t"]), T(s["normals"]), T(s["radii"]))
    n_in = T(s["normals"])
    for img, exact in ((flat, False), (away, True)):
        obj = objects.VirtualObject(s["v"], s["f"], device=dev(), uv=s["uv"], face_uv=s["fuv"],
                                    normal_map=objects.Texture(img, device=dev()))
        got = objects.sample_textures(obj, *args)
        assert set(got) == {"lod", "normals"}
        deg = T(s["mask"] & (s["face"] == 5), torch.bool)
        assert bool(deg.any()) and bits_equal(got["normals"][deg], n_in[deg])  # det == 0: N, bit for bit
        k = T(keep, torch.bool)
        if exact:
            assert bits_equal(got["normals"][k], n_in[k])
        else:
            err = float((got["normals"][k] - n_in[k]).abs().max())
            print("flat normal map: max |n - N| =", err)
            assert err <= TOL
        assert bool((got["normals"][~T(s["mask"], torch.bool)] == 0).all())


# ---------------------------------------------------------------------------------------------------- 4. composition
def make_model():
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    model = pn.PanoMipNeRF(num_samples=16, rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    model.mlp.load_state_dict(orc.init_params(4, 5))
    model = model.to(dev())
    model.mlp_mode = "fused_f16x2"
    return model


def quad(textured):
    from pano_nerf_amd import objects
    v = np.array([[-0.25, -0.2, -0.6], [0.25, -0.2, -0.55], [0.25, 0.2, -0.6], [-0.25, 0.2, -0.65]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    kw = {}
    if textured:
        rng = np.random.default_rng(5)
        yy, xx = np.mgrid[0:32, 0:32]
        checker = np.where(((yy // 16 + xx // 16) % 2)[..., None] == 0, np.uint8(230), np.uint8(30)) * np.ones((1, 1, 3), np.uint8)
        rough = (0.2 + 0.6 * rng.random((8, 8))).astype(np.float32)
        nm = np.concatenate([0.5 + 0.3 * (rng.random((16, 16, 2)) - 0.5), np.ones((16, 16, 1))], 2).astype(np.float32)
        kw = dict(uv=np.array([[0, 0], [2, 0], [2, 2], [0, 2]], np.float32),
                  albedo_map=objects.Texture(checker.astype(np.uint8), srgb=True, device=dev()),
                  roughness_map=objects.Texture(rough, device=dev()), normal_map=objects.Texture(nm, device=dev()))
    return objects.VirtualObject(v, f, albedo=(0.6, 0.5, 0.4), roughness=0.4, device=dev(), **kw)


def by_hand(model, camera, c2w, obj, accel, textured):
    """insert_object composed from the public pieces"""
    import pano_nerf_amd as pn
    from pano_nerf_amd import lighting, objects, views
    H, W = camera.h, camera.w
    scene_ = views.render_view(model, camera, c2w, outputs=("rgb", "depth", "normal"))
    rows = lambda x: x.permute(0, 2, 3, 1).reshape(H * W, -1)
    s_rgb, s_dep, s_nor = rows(scene_["fine_rgb"]), rows(scene_["fine_dep"]), rows(scene_["fine_nor"])
    probes = lighting.light_probes(model, obj.centroid(), 8, 16)
    rays = pn.generate_pano_rays(H, W, c2w) if isinstance(camera, views.PanoCamera) else \
        views.generate_perspective_rays(camera, c2w)
    t, face, bary = objects.trace_mesh(rays.origins, rays.directions, obj.vertices, obj.faces, accel=accel)
    if textured:
        at = objects.hit_attributes(obj, rays.origins, rays.directions, t, face, bary, s_dep, radii=rays.radii)
    else:
        at = objects.hit_attributes(obj, rays.origins, rays.directions, t, face, bary, s_dep)
    m = at["mask"]
    object_rgb = torch.zeros(H * W, 3, device=dev())
    assert bool(m.any())
    rough = at["roughness"][m] if textured else obj.roughness
    object_rgb[m] = objects.shade(probes, at["albedo"][m], at["normals"][m], at["viewdirs"][m], rough)[0]
    sprobe = lighting.light_probes(model, obj.centroid(), 8, 16)
    shadow = objects.shadow_ratio(at["scene_points"], s_nor, sprobe, obj.vertices, obj.faces, 1e-3, accel=accel)
    rgb = torch.where(m[:, None], object_rgb, s_rgb * shadow[:, None])
    depth = torch.where(m, t, s_dep[:, 0])
    img = lambda x: x.reshape(1, H, W, -1).permute(0, 3, 1, 2)
    return dict(mask=img(m.float()), object_rgb=img(object_rgb), shadow=img(shadow), rgb=img(rgb), depth=img(depth)), at


@pytest.mark.parametrize("cam", ["pinhole", "pano"])
def test_insert_object_with_textures_is_the_composition_of_its_pieces(cam):
    from pano_nerf_amd import objects, views
    model = make_model()
    camera = views.perspective_camera(24, 32, fov_x_deg=60.0) if cam == "pinhole" else views.pano_camera(32, 64)
    c2w = views.look_at((0.1, 0.05, 0.2), (0.0, 0.0, -0.6))
    tex, plain = quad(True), quad(False)
    outs = {}
    for accel in (None, "bvh"):
        out = objects.insert_object(model, camera, c2w, tex, probe_size=(8, 16), accel=accel)
        want, at = by_hand(model, camera, c2w, tex, accel, True)
        assert set(at) >= {"roughness", "albedo", "normals"} and tuple(at["roughness"].shape) == (camera.h * camera.w, 1)
        for k in want:
            assert bits_equal(out[k], want[k]), (cam, accel, k)
        outs[accel] = out
        # the same object without maps: the untextured path, bit for bit, and another picture
        out0 = objects.insert_object(model, camera, c2w, plain, probe_size=(8, 16), accel=accel)
        want0, at0 = by_hand(model, camera, c2w, plain, accel, False)
        assert "roughness" not in at0
        for k in want0:
            assert bits_equal(out0[k], want0[k]), (cam, accel, k, "plain")
        assert bits_equal(out0["mask"], out["mask"]) and not bits_equal(out0["object_rgb"], out["object_rgb"])
    m = outs[None]["mask"][0, 0] > 0
    print(cam, "masked pixels:", int(m.sum()), "of", m.numel())
    assert int(m.sum()) > 8 and bool(torch.isfinite(outs[None]["object_rgb"]).all())
    # the maps show: albedo varies over the quad (the checkerboard), roughness stays in the map's range, normals are unit
    a = at["albedo"][at["mask"]]
    assert float(a.max()) - float(a.min()) > 0.2
    r = at["roughness"][at["mask"]]
    assert 0.2 <= float(r.min()) and float(r.max()) <= 0.8
    assert float((at["normals"][at["mask"]].norm(dim=1) - 1).abs().max()) < 1e-6
    # transformed() carries the maps along
    moved = tex.transformed(np.eye(4))
    assert moved.albedo_map is tex.albedo_map and moved.normal_map is tex.normal_map and bits_equal(moved.uv, tex.uv)
    out2 = objects.insert_object(model, camera, c2w, moved, probe_size=(8, 16))
    assert bits_equal(out2["object_rgb"], outs[None]["object_rgb"])


def test_from_obj_loads_the_material_maps(tmp_path):
    from pano_nerf_amd import io_exr, objects
    rng = np.random.default_rng(2)
    kd = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
    io_exr.write_png(str(tmp_path / "kd.png"), kd)
    io_exr.write_exr(str(tmp_path / "pr.exr"), rng.random((2, 2, 3)).astype(np.float32))
    (tmp_path / "q.mtl").write_text("newmtl m\nKd 0.1 0.2 0.3\nmap_Kd kd.png\nmap_Pr pr.exr\n\nnewmtl other\nKd 1 1 1\n")
    (tmp_path / "q.obj").write_text("mtllib q.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\n"
                                    "usemtl m\nf 1/1 2/2 3/3 4/4\n")
    obj = objects.VirtualObject.from_obj(str(tmp_path / "q.obj"), device=dev())
    assert obj.albedo == (0.1, 0.2, 0.3) and obj.roughness == 1.0 and obj.normal_map is None
    assert obj.faces.shape == (2, 3) and obj.face_uv.shape == (2, 3) and obj.flip_v and obj.wrap == "repeat"
    assert bits_equal(obj.albedo_map.data, objects.Texture(kd, srgb=True, device=dev()).data)
    assert (obj.roughness_map.H, obj.roughness_map.W, obj.roughness_map.srgb) == (2, 2, False)
    # flip_v: V = 0 is the image's last row - the hit at the corner (u, v) = (0, 0) of face 0 reads near texel (3, 0)
    got = objects.sample_textures(obj, T([True], torch.bool), T([0], torch.int32), T([[0.0, 0.0]]),
                                  T([[0.0, 0.0, -1.0]]), T([1.0]), T([[0.0, 0.0, 1.0]]))
    levels = ref.pyramid(ref.level0(kd, True))
    want = ref.bilinear(levels[0], 0.0, 1.0, "repeat")[:3]
    assert np.abs(N(got["albedo"])[0] - want).max() <= TOL
    (tmp_path / "two.obj").write_text("mtllib q.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nusemtl m\nf 1/1 2/1 3/1\n"
                                      "usemtl other\nf 1/1 3/1 4/1\n")
    with pytest.raises(ValueError, match="'m', 'other'"):
        objects.VirtualObject.from_obj(str(tmp_path / "two.obj"), device=dev())
    other = objects.VirtualObject.from_obj(str(tmp_path / "two.obj"), material="other", device=dev())
    assert other.faces.tolist() == [[0, 2, 3]] and other.albedo == (1.0, 1.0, 1.0) and not other.textured
    with pytest.raises(ValueError, match="no material 'x'"):
        objects.VirtualObject.from_obj(str(tmp_path / "two.obj"), material="x", device=dev())


# ------------------------------------------------------------------------------------------------ 5. argument errors
def test_argument_errors(tmp_path):
    from pano_nerf_amd import _lib, objects
    s = scene()
    tex = objects.Texture(np.zeros((2, 2, 3), np.float32), device=dev())
    grey = objects.Texture(np.zeros((2, 2), np.uint8), device=dev())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objects.Texture(torch.zeros(2, 2, 3))
    with pytest.raises(ValueError, match="C in"):
        objects.Texture(np.zeros((2, 2, 2), np.float32), device=dev())
    with pytest.raises(ValueError, match="uint8 or floating"):
        objects.Texture(np.zeros((2, 2, 3), np.int32), device=dev())
    with pytest.raises(ValueError, match="srgb"):
        objects.Texture(np.zeros((2, 2, 3), np.float32), srgb=True, device=dev())
    with pytest.raises(ValueError, match="level 2"):
        tex.level(2)
    with pytest.raises(ValueError, match=".png and .exr"):
        objects.Texture.from_file(str(tmp_path / "x.jpg"))
    v, f, uv, fuv = s["v"], s["f"], s["uv"][:13], np.where(s["fuv"] > 12, 12, s["fuv"])
    mk = lambda **kw: objects.VirtualObject(v, f, device=dev(), **kw)
    with pytest.raises(ValueError, match="albedo_map needs uv"):
        mk(albedo_map=tex)
    with pytest.raises(ValueError, match="must be a Texture"):
        mk(uv=uv, face_uv=fuv, normal_map=np.zeros((2, 2, 3)))
    with pytest.raises(ValueError, match="face_uv index outside the 13 uv rows"):
        mk(uv=uv, face_uv=s["fuv"])
    with pytest.raises(ValueError, match="face_uv must be"):
        mk(uv=uv, face_uv=fuv[:3])
    with pytest.raises(ValueError, match="per vertex"):
        mk(uv=uv)
    with pytest.raises(ValueError, match="face_uv needs uv"):
        mk(face_uv=fuv)
    with pytest.raises(ValueError, match=r"uv must be \[T, 2\]"):
        mk(uv=np.zeros((7, 3), np.float32))
    with pytest.raises(ValueError, match="roughness_map needs roughness"):
        mk(uv=uv, face_uv=fuv, roughness_map=tex)
    with pytest.raises(ValueError, match="albedo_map needs 3 channels"):
        mk(uv=uv, face_uv=fuv, albedo_map=grey)
    with pytest.raises(ValueError, match="wrap must be"):
        mk(uv=uv, face_uv=fuv, albedo_map=tex, wrap="mirror")
    obj = mk(uv=uv, face_uv=fuv, albedo_map=tex, roughness=0.3, roughness_map=grey)
    assert obj.textured and not mk(uv=uv, face_uv=fuv).textured
    R = 4
    z3, z2, z1 = torch.zeros(R, 3, device=dev()), torch.zeros(R, 2, device=dev()), torch.zeros(R, device=dev())
    zi, zm = torch.zeros(R, dtype=torch.int32, device=dev()), torch.ones(R, dtype=torch.bool, device=dev())
    with pytest.raises(ValueError, match="at least one texture map"):
        objects.sample_textures(mk(uv=uv, face_uv=fuv), zm, zi, z2, z3, z1, z3)
    with pytest.raises(ValueError, match="radii must be"):
        objects.sample_textures(obj, zm, zi, z2, z3, z1, z3, radii=z1[:3])
    with pytest.raises(ValueError, match="must match the 4 rows"):
        objects.sample_textures(obj, zm, zi[:2], z2, z3, z1, z3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objects.sample_textures(obj, zm, zi, z2, z3, z1, z3.cpu())
    with pytest.raises(ValueError, match="radii must be"):
        objects.hit_attributes(obj, z3, z3, z1, zi, z2, radii=torch.zeros(R, 2, device=dev()))
    assert objects.sample_textures(obj, zm[:0], zi[:0], z2[:0], z3[:0], z1[:0], z3[:0])["albedo"].shape == (0, 3)
    # the C entry points check shapes and pointers before they launch
    lib = _lib.load()
    buf = torch.zeros(64, device=dev())
    assert lib.pn_tex_floats(16384, 16384) == 4 * sum((16384 >> l) ** 2 for l in range(15)) and lib.pn_tex_floats(16385, 1) < 0
    for args, what in (((0, 2, 3, 0, buf.data_ptr(), None, buf.data_ptr(), None), "bad shape"),
                       ((2, 2, 5, 0, buf.data_ptr(), None, buf.data_ptr(), None), "bad shape"),
                       ((2, 2, 3, 1, buf.data_ptr(), None, buf.data_ptr(), None), "null"),
                       ((2, 2, 3, 0, None, None, buf.data_ptr(), None), "null")):
        code = lib.pn_tex_ingest(*args)
        assert code != 0 and what in lib.pn_strerror(code).decode().lower(), (args, lib.pn_strerror(code))
    assert lib.pn_tex_pyramid(2, 0, buf.data_ptr(), None) != 0 and lib.pn_tex_pyramid(2, 2, None, None) != 0
