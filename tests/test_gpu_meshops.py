"""The mesh operations on the GPU against the numpy restatement of tests/_meshops_ref.py: components (labels, records,
filtering), quadric vertex clustering on the shared meshes and on a marching-tetrahedra sphere, edge inputs, the face-count
target, the edge census, and the composition of export_scene / fused_mesh with the two new arguments.

Tolerance (from the number formats).  Both sides evaluate the header's formulas in fp64 on the same fp32 inputs in the
same order and round once; +, -, *, / and sqrt are correctly rounded on both, and the library builds with
-ffp-contract=off.  Away from the discrete decisions the restatement marks fragile (at most 1 % of a mesh's clusters, capped
in test_meshops_cpu.py and here for the device-made sphere; in fact none) the fp64 values agree to the bit, and
test_meshops_cpu.py shows that even another order moves them by less than 1e-12 cell: every fp32 output is held to ONE
fp32 ulp of the reference and every integer output exactly.  Each comparison prints the worst ulp distance it saw."""
import functools

import numpy as np
import pytest
import torch

import _meshops_ref as ref

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def T(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(dev())


def N(x):
    return x.detach().cpu().numpy()


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def ulps(got, want, rows=None):
    """the worst distance of the fp32 `got` from the fp64 `want` in fp32 ulps of `want`"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = np.abs(got - want) / ulp32(want)
    if rows is not None:
        d = d[rows]
    return float(d.max()) if d.size else 0.0


def mesh_of(v, f, normals=None, colors=None):
    from pano_nerf_amd.geometry import Mesh
    g = lambda t: None if t is None else T(t)
    return Mesh(T(v), T(f), g(normals), g(colors))


@functools.lru_cache(maxsize=None)
def cases():
    return ref.component_cases()


# ------------------------------------------------------------------------------------------------------ components
@pytest.mark.parametrize("name", list(ref.component_cases()))
def test_components(name):
    from pano_nerf_amd import meshops
    v, f = cases()[name]
    want_v, want_f, want_c = ref.components(f, len(v))
    vlab, flab, count = meshops.mesh_components(T(f), len(v))
    assert count == want_c and vlab.dtype == torch.int32 and flab.dtype == torch.int32
    assert np.array_equal(N(vlab), want_v) and np.array_equal(N(flab), want_f)
    again = meshops.mesh_components(T(f), len(v))
    assert bits_equal(again[0], vlab) and bits_equal(again[1], flab) and again[2] == count
    st = meshops.component_stats(T(v), T(f), flab, count)
    want = ref.component_stats(v, f, want_f, want_v, want_c)
    assert np.array_equal(N(st["faces"]), want["faces"]) and np.array_equal(N(st["vertices"]), want["vertices"])
    assert np.array_equal(N(st["bbox"]), want["bbox"])
    worst = max(ulps(N(st["area"]), want["area"]), ulps(N(st["volume"]), want["volume"]))
    print(f"components {name}: {count} components, worst {worst:.3f} ulp32")
    assert worst <= 1.0
    st2 = meshops.component_stats(T(v), T(f), flab, count)
    assert all(bits_equal(st[k], st2[k]) for k in st)


@pytest.mark.parametrize("kw", [dict(min_faces=5), dict(keep_largest=1), dict(keep_largest=2, by="faces", min_area=1.0),
                                dict(keep_largest=1, by="volume"), dict(min_area=1000.0)],
                         ids=["min_faces", "largest", "two_by_faces", "by_volume", "nothing_left"])
def test_filter_components(kw):
    from pano_nerf_amd import meshops
    v, f = cases()["spheres_floater"]
    nrm, col = ref.attributes(v)
    (wv, wf, wn, wc), wvm, wfm = ref.filter_components(v, f, normals=nrm, colors=col, **kw)
    out, vmap, fmap = meshops.filter_components(mesh_of(v, f, nrm, col), **kw)
    assert np.array_equal(N(vmap), wvm) and np.array_equal(N(fmap), wfm) and np.array_equal(N(out.faces), wf)
    assert bits_equal(out.vertices, torch.from_numpy(wv)) and bits_equal(out.normals, torch.from_numpy(wn))
    assert bits_equal(out.colors, torch.from_numpy(wc))
    assert out.faces.dtype == torch.int32 and vmap.dtype == torch.int32 and fmap.dtype == torch.int32


def test_filter_components_on_every_case():
    from pano_nerf_amd import meshops
    for name, (v, f) in cases().items():
        (wv, wf, _, _), wvm, wfm = ref.filter_components(v, f, min_faces=2, keep_largest=1)
        out, vmap, fmap = meshops.filter_components((T(v), T(f)), min_faces=2, keep_largest=1)
        assert np.array_equal(N(vmap), wvm) and np.array_equal(N(fmap), wfm) and np.array_equal(N(out.faces), wf), name
        assert bits_equal(out.vertices, torch.from_numpy(wv)), name


# --------------------------------------------------------------------------------------------------- simplification
def check_simplify(v, f, cell, origin, what, normals=None, colors=None):
    from pano_nerf_amd import meshops
    want = ref.simplify(v, f, cell, origin, normals=normals, colors=colors)
    assert want["fragile_all"].mean() <= 0.01, what
    m = mesh_of(v, f, normals, colors)
    out, vmap, fmap, flags, info = meshops.simplify_mesh(m, cell=cell, origin=origin, return_info=True)
    assert info["cell"] == want["cell"] and list(info["n"]) == list(want["n"]) and np.array_equal(np.float32(info["lo"]), want["lo"])
    assert np.array_equal(N(info["keys"]), want["keys"]) and np.array_equal(N(info["cluster_keys"]), want["cluster_keys"])
    assert np.array_equal(N(info["rank"]), want["rank"])
    assert np.array_equal(N(vmap), want["vertex_map"]) and np.array_equal(N(fmap), want["face_map"])
    assert np.array_equal(N(out.faces), want["faces"])
    ok = ~want["fragile"]
    assert flags.dtype == torch.uint8 and np.array_equal(N(flags)[ok], want["flags"][ok])
    worst = ulps(N(out.vertices), want["vertices"], ok)
    if normals is not None:
        worst = max(worst, ulps(N(out.normals), want["normals"]), ulps(N(out.colors), want["colors"]))
    print(f"simplify {what}: {len(v)} -> {len(want['vertices'])} vertices, {len(f)} -> {len(want['faces'])} faces, "
          f"{int((want['flags'] == 1).sum())} fallbacks, {int((~ok).sum())} fragile, worst {worst:.3f} ulp32")
    assert worst <= 1.0
    again = meshops.simplify_mesh(m, cell=cell, origin=origin)
    assert bits_equal(again[0].vertices, out.vertices) and bits_equal(again[0].faces, out.faces)
    assert bits_equal(again[0].normals, out.normals) and bits_equal(again[0].colors, out.colors)
    assert bits_equal(again[1], vmap) and bits_equal(again[2], fmap) and bits_equal(again[3], flags)
    assert meshops.edge_counts(out.faces) == ref.edge_counts(want["faces"])
    return out, want


@pytest.mark.parametrize("name,cell", ref.SIMPLIFY_CASES, ids=[f"{n}-{c}" for n, c in ref.SIMPLIFY_CASES])
def test_simplify_against_the_reference(name, cell):
    v, f, origin = ref.simplify_case(name)
    nrm, col = ref.attributes(v)
    check_simplify(v, f, cell, origin, f"{name}-{cell}", nrm, col)


@pytest.mark.parametrize("cells", [2, 4])
def test_simplify_marching_tetrahedra_sphere(cells):
    """the mesh marching_tetrahedra makes of an analytic sphere volume at 48^3, clustered at 2 and 4 grid steps"""
    from pano_nerf_amd import geometry, meshops
    n, R = 48, 0.8
    bounds = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    x = torch.linspace(-1.0, 1.0, n, device=dev())
    gx, gy, gz = torch.meshgrid(x, x + 0.013, x - 0.007, indexing="ij")
    vol = R - torch.sqrt(gx * gx + gy * gy + gz * gz)
    verts, faces = geometry.marching_tetrahedra(vol, 0.0, bounds)
    assert faces.shape[0] > 10000
    h = 2.0 / (n - 1)
    out, want = check_simplify(N(verts), N(faces), cells * h, None, f"mt-sphere-{cells}h")
    assert out.faces.shape[0] < faces.shape[0] // cells
    assert meshops.edge_counts(faces) == {"boundary": 0, "nonmanifold": 0, "inconsistent": 0}


def test_edge_inputs():
    from pano_nerf_amd import meshops
    # all vertices in one cell: nothing survives
    v, f = cases()["fans"]
    out, vmap, fmap, flags = meshops.simplify_mesh((T(v), T(f)), cell=16.0)
    assert tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and fmap.numel() == 0 and flags.numel() == 0
    assert bool((vmap == -1).all()) and vmap.shape[0] == len(v)
    # vertices exactly on cell walls: the cube with the default origin, cell 0.25 = two grid steps
    cv, cf = ref.cube()
    want = ref.simplify(cv, cf, 0.25)
    got = meshops.simplify_mesh((T(cv), T(cf)), cell=0.25, return_info=True)
    assert np.array_equal(N(got[4]["keys"]), want["keys"]) and np.array_equal(N(got[0].faces), want["faces"])
    assert np.array_equal(N(got[1]), want["vertex_map"]) and np.array_equal(N(got[2]), want["face_map"])
    ok = ~want["fragile"]
    assert ok.any() and np.array_equal(N(got[3])[ok], want["flags"][ok])
    assert ulps(N(got[0].vertices), want["vertices"], ok) <= 1.0
    # a face with a repeated index and a zero-area face (three collinear vertices): the first is dropped whatever the
    # cell, the second adds nothing to any quadric
    v2 = np.concatenate([cv, ref.f32([[2.0, 2.0, 2.0], [2.5, 2.5, 2.5], [3.0, 3.0, 3.0]])])
    k = len(cv)
    f2 = np.concatenate([cf, np.asarray([[0, 0, 5], [k, k + 1, k + 2]], np.int32)])
    origin = ref.f32(v2.min(0).astype(np.float64) - 0.01)
    want = ref.simplify(v2, f2, 0.3, origin)
    out, vmap, fmap, flags = meshops.simplify_mesh((T(v2), T(f2)), cell=0.3, origin=origin)
    assert np.array_equal(N(out.faces), want["faces"]) and np.array_equal(N(fmap), want["face_map"])
    assert len(cf) not in N(fmap) and len(cf) + 1 in N(fmap)
    assert not want["fragile"].any() and np.array_equal(N(flags), want["flags"]) and (want["flags"] == 2).sum() == 3
    assert ulps(N(out.vertices), want["vertices"]) <= 1.0
    # the empty mesh passes through everywhere
    e_v, e_f = T(np.zeros((0, 3), np.float32)), T(np.zeros((0, 3), np.int32))
    out, vmap, fmap, flags = meshops.simplify_mesh((e_v, e_f), cell=1.0)
    assert out.vertices.shape[0] == 0 and out.faces.shape[0] == 0 and vmap.numel() == 0
    out, vmap, fmap = meshops.filter_components((e_v, e_f), min_faces=3)
    assert out.vertices.shape[0] == 0 and out.faces.shape[0] == 0
    assert meshops.mesh_components(e_f, 0)[2] == 0
    assert meshops.edge_counts(e_f) == {"boundary": 0, "nonmanifold": 0, "inconsistent": 0}


def test_argument_errors():
    from pano_nerf_amd import meshops
    v, f = cases()["fans"]
    tv, tf = T(v), T(f)
    with pytest.raises(ValueError, match="2\\^21"):  # a Python-side raise: far more clusters than the face keys hold
        big_v, big_f = ref.icosphere(4, 1.0)
        sv = np.concatenate([big_v * np.float32(s) for s in np.linspace(1.0, 60.0, 900)])
        meshops.simplify_mesh((T(sv), T(big_f)), cell=1e-4)
    with pytest.raises(ValueError, match="63 bits"):
        meshops.simplify_mesh((tv, tf), cell=1e-30)
    with pytest.raises(RuntimeError, match="HIP device only"):
        meshops.simplify_mesh((torch.from_numpy(v), torch.from_numpy(f)), cell=0.5)
    with pytest.raises(RuntimeError, match="HIP device only"):
        meshops.mesh_components(torch.from_numpy(f), len(v))
    with pytest.raises(RuntimeError, match="HIP device only"):
        meshops.filter_components((torch.from_numpy(v), torch.from_numpy(f)))
    with pytest.raises(RuntimeError, match="HIP device only"):
        meshops.edge_counts(torch.from_numpy(f))
    with pytest.raises(ValueError, match="int32"):
        meshops.simplify_mesh((tv, tf.to(torch.int64)), cell=0.5)
    with pytest.raises(ValueError, match="float32"):
        meshops.simplify_mesh((tv.to(torch.float64), tf), cell=0.5)
    with pytest.raises(ValueError, match="int32"):
        meshops.mesh_components(tf.to(torch.int64), len(v))
    with pytest.raises(ValueError, match="exactly one"):
        meshops.simplify_mesh((tv, tf))
    with pytest.raises(ValueError, match="exactly one"):
        meshops.simplify_mesh((tv, tf), cell=0.5, target_faces=4)
    with pytest.raises(ValueError, match="cell must be"):
        meshops.simplify_mesh((tv, tf), cell=0.0)
    bad = v.copy()
    bad[3, 1] = np.nan
    for fn in (lambda m: meshops.simplify_mesh(m, cell=0.5), meshops.filter_components):
        with pytest.raises(ValueError, match="NaN"):
            fn((T(bad), tf))
    out_of_range = f.copy()
    out_of_range[2, 1] = len(v)
    for fn in (lambda m: meshops.simplify_mesh(m, cell=0.5), meshops.filter_components,
               lambda m: meshops.mesh_components(m[1], len(v))):
        with pytest.raises(ValueError, match="outside"):
            fn((tv, T(out_of_range)))
    out_of_range[2, 1] = -1
    with pytest.raises(ValueError, match="outside"):
        meshops.mesh_components(T(out_of_range), len(v))
    with pytest.raises(ValueError, match="by must be"):
        meshops.filter_components((tv, tf), by="weight")


@pytest.mark.parametrize("target", [100, 700])
def test_target_faces(target):
    from pano_nerf_amd import meshops
    v, f, _ = ref.simplify_case("ico")
    m = (T(v), T(f))
    out, vmap, fmap, flags, info = meshops.simplify_mesh(m, target_faces=target, return_info=True)
    assert 0 < out.faces.shape[0] <= target
    same = meshops.simplify_mesh(m, cell=info["cell"])
    assert bits_equal(same[0].vertices, out.vertices) and bits_equal(same[0].faces, out.faces)
    assert bits_equal(same[1], vmap) and bits_equal(same[2], fmap) and bits_equal(same[3], flags)
    want = ref.simplify(v, f, info["cell"])
    assert np.array_equal(N(out.faces), want["faces"])
    print(f"target {target}: cell {info['cell']:.4f}, {out.faces.shape[0]} faces")


# ------------------------------------------------------------------------------------------------------ 7. plumbing
@functools.lru_cache(maxsize=None)
def model():
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    m = pn.PanoMipNeRF(num_samples=8, rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    m.mlp.load_state_dict(orc.init_params(4, 5))
    return m.to(dev())


class Recorder:
    """wraps _lib.call and lists the entry points called"""

    def __init__(self, monkeypatch):
        from pano_nerf_amd import _lib
        self.names = []
        real = _lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)

        monkeypatch.setattr(_lib, "call", call)

    def take(self):
        out, self.names = self.names, []
        return out


NEW = ("pn_mesh_", "pn_cluster_")


def test_export_scene_composes(tmp_path, monkeypatch):
    from pano_nerf_amd import geometry, meshops
    bounds, res = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), 10
    sigma = geometry.density_grid(model(), bounds, res)
    level = float(sigma.median())
    rec = Recorder(monkeypatch)
    # with both arguments None: what the function did before they existed - the same entry points in the same order as
    # the composition of the untouched parts, none of the new ones, and the same bits
    plain = geometry.export_scene(model(), bounds, res, level, str(tmp_path / "a.obj"), size=512)
    seq = rec.take()
    assert seq and not [n for n in seq if n.startswith(NEW)]
    verts, faces = geometry.marching_tetrahedra(geometry.density_grid(model(), bounds, res), level, bounds)
    var = max(geometry._placement(bounds, (res,) * 3)[1]) ** 2 / 12.0
    hand = geometry.bake_textures(model(), geometry._field_mesh(model(), verts, faces, var, True, None, None), size=512)
    geometry.write_obj(str(tmp_path / "b.obj"), hand)
    assert rec.take() == seq
    for a, b in ((plain.vertices, hand.vertices), (plain.faces, hand.faces), (plain.normals, hand.normals), (plain.uv, hand.uv)):
        assert bits_equal(a, b)
    assert all(bits_equal(plain.maps[k], hand.maps[k]) for k in hand.maps)
    for ext in ("obj", "mtl"):
        assert (tmp_path / f"a.{ext}").read_text().replace("a.mtl", "b.mtl").replace("a_", "b_").replace(" a\n", " b\n") == \
            (tmp_path / f"b.{ext}").read_text()
    # with them: extract, filter_components, simplify_mesh, the field at the new vertices, bake - bit for bit
    assert faces.shape[0] > 0
    h = 2.0 / (res - 1)
    got = geometry.export_scene(model(), bounds, res, level, str(tmp_path / "c.obj"), size=512, simplify=2 * h,
                                min_component_faces=4)
    assert [n for n in rec.take() if n.startswith(NEW)]
    m = meshops.filter_components((verts, faces), min_faces=4)[0]
    m = meshops.simplify_mesh(m, cell=2 * h)[0]
    hand = geometry.bake_textures(model(), geometry._field_mesh(model(), m.vertices, m.faces, var, True, None, None), size=512)
    for a, b in ((got.vertices, hand.vertices), (got.faces, hand.faces), (got.normals, hand.normals), (got.uv, hand.uv)):
        assert bits_equal(a, b)
    assert all(bits_equal(got.maps[k], hand.maps[k]) for k in hand.maps)
    assert got.faces.shape[0] < faces.shape[0]
    by_target = geometry.extract_mesh(model(), bounds, res, level, simplify={"target_faces": 40})
    assert by_target.faces.shape[0] <= 40 and by_target.normals.shape == by_target.vertices.shape


def test_fused_mesh_composes(monkeypatch):
    from pano_nerf_amd import fusion, geometry, meshops, views
    # a volume whose surface does not depend on the model: a constant-depth panorama, i.e. a sphere of radius 0.4
    cam = views.pano_camera(16, 32)
    bounds, res = ((-0.6, -0.5, -0.55), (0.5, 0.6, 0.45)), 12
    vol = fusion.TSDFVolume(bounds, res, device=dev())
    vol.integrate(torch.full((1, 16, 32), 0.4, device=dev()), cam, np.eye(4))
    verts, faces = vol.mesh()
    rec = Recorder(monkeypatch)
    plain = fusion.fused_mesh(model(), vol, colors="albedo")
    seq = rec.take()
    assert not [n for n in seq if n.startswith(NEW)]
    var = max(vol.step) ** 2 / 12.0
    vol.mesh()
    hand = geometry._field_mesh(model(), verts, faces, var, True, "albedo", None)
    assert rec.take() == seq
    assert bits_equal(plain.vertices, hand.vertices) and bits_equal(plain.faces, hand.faces)
    assert bits_equal(plain.normals, hand.normals) and bits_equal(plain.colors, hand.colors)
    assert faces.shape[0] > 100
    cell = 2.0 * max(vol.step)
    got = fusion.fused_mesh(model(), vol, colors="albedo", simplify={"cell": cell}, min_component_faces=2)
    assert [n for n in rec.take() if n.startswith(NEW)]
    m = meshops.filter_components((verts, faces), min_faces=2)[0]
    m = meshops.simplify_mesh(m, cell=cell)[0]
    hand = geometry._field_mesh(model(), m.vertices, m.faces, var, True, "albedo", None)
    assert bits_equal(got.vertices, hand.vertices) and bits_equal(got.faces, hand.faces)
    assert bits_equal(got.normals, hand.normals) and bits_equal(got.colors, hand.colors)
    assert got.faces.shape[0] < faces.shape[0]
