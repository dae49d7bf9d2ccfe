"""The device-built BVH and the tracers that walk it: trees against test_bvh_cpu.py's checker, trace_mesh(accel=...) against
its numpy restatement of the contract bit for bit and against the brute-force kernel bit for bit, shadow_ratio and
insert_object against their brute-force selves, and the plumbing (one build per path, the cache, the untouched default).
Everything here is an equality of bits: there are no tolerances."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _load(name, file):
    s = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), file))
    m = importlib.util.module_from_spec(s)
    s.loader.exec_module(m)
    return m


bspec = _load("_bvh_spec", "test_bvh_cpu.py")
gobj = _load("_gpu_objects_helpers", "test_gpu_objects.py")
spec = bspec.spec
T, N, bits_equal, dev = gobj.T, gobj.N, gobj.bits_equal, gobj.dev
CENTRE, RADIUS, EYE = bspec.CENTRE, bspec.RADIUS, bspec.EYE
f32 = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32) if a.dtype == f32 else a,
                                                                        b.view(np.int32) if b.dtype == f32 else b)


class Recorder:
    """Counts the entry points that go through _lib.call."""

    def __init__(self, monkeypatch):
        from pano_nerf_amd import _lib
        self.names = []
        real = _lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)

        monkeypatch.setattr(_lib, "call", call)

    def bvh(self):
        return [n for n in self.names if "bvh" in n]


_ICO6 = []


def ico6():
    if not _ICO6:
        _ICO6.append(spec.icosphere(6, RADIUS, CENTRE))
    return _ICO6[0]


# ------------------------------------------------------------------------------------------------------------- trees
def _tree_mesh(kind):
    if kind == "stack":  # 4096 triangles (p, -p, 0) around the origin: fp32 negation is exact, so every box is [-a, a], every
        rng = np.random.default_rng(2)  # centre is exactly 0, every key is the same and the sorted position alone splits them
        F = 4096
        off = (rng.normal(size=(F, 3)) * 0.1).astype(f32)
        v = np.concatenate([off, -off, np.zeros((F, 3), f32)])
        lo = np.stack([np.arange(F), np.arange(F) + F, np.arange(F) + 2 * F], 1).astype(np.int32)
        return v, lo
    if kind == "bad":
        v, f = spec.icosphere(3, RADIUS, CENTRE)
        f = f.copy()
        f[::3, 1] = len(v) + 7
        f[5, 0] = -1
        return v, f
    if kind == 81920:
        return ico6()
    v, f = spec.icosphere(3, RADIUS, CENTRE)
    return v, f[:kind]


@pytest.mark.parametrize("kind", [1, 2, 3, 1280, 81920, "stack", "bad"])
def test_device_trees_are_valid_and_builds_repeat(kind):
    from pano_nerf_amd import objects
    v, f = _tree_mesh(kind)
    F = len(f)
    tv, tf = T(v), T(f, torch.int32)
    bvh = objects.MeshBVH.build(tv, tf)
    assert bvh.F == F and bvh.nodes.shape == (max(F - 1, 1), 16) and bvh.tris.shape == (F, 12) and bvh.device == dev()
    lo, hi = bspec.tri_boxes(v, f)
    depth = bspec.check_tree(N(bvh.nodes), F, lo, hi)
    print(kind, "faces", F, "internal nodes above the deepest leaf:", depth)
    assert depth <= bspec.KEY_BITS + max(F - 1, 1).bit_length()
    if kind == "stack":
        assert np.array_equal(lo, -hi) and not (f32(0.5) * lo + f32(0.5) * hi).any()  # the centres are one point, exactly
        from pano_nerf_amd import _lib
        tbox = torch.zeros(F, 2, 4, device=dev())
        tbox[:, 0, :3], tbox[:, 1, :3] = T(lo), T(hi)
        scene = torch.cat([T(lo).amin(0), T(hi).amax(0)]).contiguous()
        keys = torch.empty(F, dtype=torch.int64, device=dev())
        _lib.call("pn_bvh_keys", F, tbox.data_ptr(), scene.data_ptr(), keys.data_ptr(),
                  torch.cuda.current_stream(dev()).cuda_stream)
        assert int(keys.min()) == int(keys.max()) >= 0  # one key: the tie-break by sorted position is all that splits
        assert depth == 12  # 4096 positions told apart by their 12 index bits alone: a complete binary tree
    if kind == "bad":
        assert np.isposinf(lo[::3]).all() and np.isposinf(lo[5]).all()
    again = objects.MeshBVH.build(tv, tf)
    assert bits_equal(again.nodes, bvh.nodes) and bits_equal(again.tris, bvh.tris)
    assert torch.equal(again.nodes.view(torch.int32), bvh.nodes.view(torch.int32))


def test_empty_meshes_and_mismatched_trees():
    from pano_nerf_amd import objects
    v, f = spec.icosphere(1, RADIUS, CENTRE)
    tv, tf = T(v), T(f, torch.int32)
    o, d = (T(x[:300]) for x in bspec.scene_rays(v, f))
    for vv, ff in ((tv, tf[:0]), (tv[:0], tf)):  # F = 0 and V = 0: nothing to hit
        empty = objects.MeshBVH.build(vv, ff)
        assert empty.F == 0 and empty.nodes is None
        for accel in ("bvh", empty):
            t, face, bary = objects.trace_mesh(o, d, vv, ff, accel=accel)
            assert bool(torch.isinf(t).all()) and bool((face == -1).all()) and bool((bary == 0).all())
            assert not bool(objects.trace_mesh(o, d, vv, ff, any_hit=True, accel=accel).any())
    assert objects.trace_mesh(o[:0], d[:0], tv, tf, accel="bvh")[0].shape == (0,)
    with pytest.raises(ValueError, match="MeshBVH of 80 faces"):
        objects.trace_mesh(o, d, tv, tf[:10], accel=objects.MeshBVH.build(tv, tf))
    with pytest.raises(ValueError, match="accel must be"):
        objects.trace_mesh(o, d, tv, tf, accel="octree")


# ------------------------------------------------------------------------------------------------------------- trace
@pytest.mark.parametrize("name", ["ico3", "soup", "sliver", "coincident", "fan"])
def test_trace_is_the_restatement_and_is_brute_force(name):
    from pano_nerf_amd import objects
    v, f = bspec.scenes()[name]
    o, d = bspec.scene_rays(v, f)
    assert len(o) % 256
    to, td, tv, tf = T(o), T(d), T(v), T(f, torch.int32)
    bvh = objects.MeshBVH.build(tv, tf)
    t, face, bary = objects.trace_mesh(to, td, tv, tf, accel=bvh)
    assert t.dtype == torch.float32 and face.dtype == torch.int32 and bary.shape == (len(o), 2)
    rt, rface, rbary, lost, accepted = bspec.candidate_trace(o, d, v, f)
    print(name, "rays", len(o), "hits", int((rface >= 0).sum()), "accepted pairs", accepted, "lost", lost)
    assert lost == 0
    assert same_bits(N(face), rface) and same_bits(N(t), rt) and same_bits(N(bary), rbary)
    bt, bface, bbary = objects.trace_mesh(to, td, tv, tf)  # brute force, every ray
    assert bits_equal(t, bt) and bits_equal(face, bface) and bits_equal(bary, bbary)
    # accel="bvh" builds the same tree for the call
    t1, face1, bary1 = objects.trace_mesh(to, td, tv, tf, accel="bvh")
    assert bits_equal(t1, t) and bits_equal(face1, face) and bits_equal(bary1, bary)
    # any_hit
    hit = objects.trace_mesh(to, td, tv, tf, any_hit=True, accel=bvh)
    assert hit.dtype == torch.bool and np.array_equal(N(hit), rface >= 0)
    # t_max: exclusive, per ray (every other ray's own t: its winner is cut away)
    tm = np.where(np.arange(len(rt)) % 2 == 0, rt, rt * f32(2)).astype(f32)
    tm[~np.isfinite(tm)] = 1.0
    t2, face2, bary2 = objects.trace_mesh(to, td, tv, tf, t_max=T(tm), accel=bvh)
    b2 = objects.trace_mesh(to, td, tv, tf, t_max=T(tm))
    assert bits_equal(t2, b2[0]) and bits_equal(face2, b2[1]) and bits_equal(bary2, b2[2])
    r2 = bspec.candidate_trace(o, d, v, f, t_max=tm)
    assert r2[3] == 0 and same_bits(N(face2), r2[1]) and same_bits(N(t2), r2[0]) and same_bits(N(bary2), r2[2])
    hit2 = objects.trace_mesh(to, td, tv, tf, t_max=T(tm), any_hit=True, accel=bvh)
    assert np.array_equal(N(hit2), r2[1] >= 0)
    # the number of rays per launch does not show, and a repeated call gives the same bits
    for R in (1, 63, 65, 1000):
        a, b, c = objects.trace_mesh(to[:R], td[:R], tv, tf, accel=bvh)
        assert bits_equal(a, t[:R]) and bits_equal(b, face[:R]) and bits_equal(c, bary[:R]), R
    a, b, c = objects.trace_mesh(to, td, tv, tf, accel=bvh)
    assert bits_equal(a, t) and bits_equal(b, face) and bits_equal(c, bary)


@pytest.mark.parametrize("rows", [(255, 256, 512), (256, 512)])
def test_equal_t_across_the_brute_force_tiles_keeps_the_lowest_face(rows):
    """One triangle three (two) times among 513 faces, the copies in different 256-triangle LDS tiles of the brute-force
    finder (255 | 256 | 512): every hit is a tie in t, and the lowest face index must win on every path.  The other faces
    are (0, 0, 0): det == 0, never hit."""
    from pano_nerf_amd import objects
    v, one = bspec.scenes()["coincident"]
    o, d = bspec.scene_rays(v, one[:1])  # aimed at the triangle itself
    f = np.zeros((513, 3), np.int32)
    f[list(rows)] = [0, 1, 2]
    assert len(o) == 18146 and len(o) % 256 and len(o) % 64
    rt, rface, rbary, lost, _ = bspec.candidate_trace(o, d, v, f)
    assert lost == 0 and int((rface >= 0).sum()) == 2529 and np.all(rface[rface >= 0] == rows[0])
    tm = np.where(rface >= 0, rt, f32(1.0)).astype(f32)  # exclusive: the winner and its equals are cut away
    assert not (bspec.candidate_trace(o, d, v, f, t_max=tm)[1] >= 0).any()
    to, td, tv, tf = T(o), T(d), T(v), T(f, torch.int32)
    for accel in (None, "bvh", objects.MeshBVH.build(tv, tf)):
        t, face, bary = objects.trace_mesh(to, td, tv, tf, accel=accel)
        assert same_bits(N(face), rface) and same_bits(N(t), rt) and same_bits(N(bary), rbary), accel
        assert np.array_equal(N(objects.trace_mesh(to, td, tv, tf, any_hit=True, accel=accel)), rface >= 0), accel
        t2, face2, bary2 = objects.trace_mesh(to, td, tv, tf, t_max=T(tm), accel=accel)
        assert bool(torch.isinf(t2).all()) and bool((face2 == -1).all()) and bool((bary2 == 0).all()), accel
        assert not bool(objects.trace_mesh(to, td, tv, tf, t_max=T(tm), any_hit=True, accel=accel).any()), accel


def test_trace_with_faces_that_index_outside_the_vertices():
    from pano_nerf_amd import objects
    v, f = _tree_mesh("bad")
    o, d = bspec.scene_rays(*spec.icosphere(3, RADIUS, CENTRE))
    o, d = o[::3], d[::3]
    got = objects.trace_mesh(T(o), T(d), T(v), T(f, torch.int32), accel="bvh")
    want = objects.trace_mesh(T(o), T(d), T(v), T(f, torch.int32))
    assert all(bits_equal(a, b) for a, b in zip(got, want))
    rt, rface, rbary, lost, _ = bspec.candidate_trace(o, d, v, f)
    assert lost == 0 and same_bits(N(got[1]), rface) and same_bits(N(got[0]), rt)
    hit = N(got[1])
    assert (hit >= 0).any() and not np.any(hit[hit >= 0] % 3 == 0)


@pytest.mark.parametrize("frame", ["pinhole 480x640", "pano 512x1024"])
def test_81920_faces_against_brute_force(frame):
    """Every ray on which the BVH and brute force differ must be the contract's doing (the numpy restatement on just those
    rays reproduces the BVH's result bit for bit), and at most 1 ray in 10^4 may differ.  Zero is expected, and zero is what
    one MI355X gave for both frames (profiles/objects_bvh.txt)."""
    from pano_nerf_amd import objects
    v, f = ico6()
    assert len(f) == 81920
    if frame.startswith("pinhole"):
        o, d = spec.pinhole_rays(480, 640, 60.0, spec.look_at(EYE, CENTRE))
    else:
        o, d = spec.pano_rays(512, 1024, EYE)
    o, d = o.astype(f32), d.astype(f32)
    to, td, tv, tf = T(o), T(d), T(v), T(f, torch.int32)
    t, face, bary = objects.trace_mesh(to, td, tv, tf, accel="bvh")
    bt, bface, bbary = objects.trace_mesh(to, td, tv, tf)
    differ = (t.view(torch.int32) != bt.view(torch.int32)) | (face != bface) | \
        (bary.view(torch.int32) != bbary.view(torch.int32)).any(1)
    idx = N(torch.nonzero(differ).reshape(-1))
    print(frame, "rays", len(o), "hits", int((face >= 0).sum()), "rays on which BVH and brute force differ:", len(idx))
    assert int((face >= 0).sum()) > 1000
    assert len(idx) <= 1e-4 * len(o), len(idx)
    if len(idx):
        rt, rface, rbary, _, _ = bspec.candidate_trace(o[idx], d[idx], v, f, chunk=16)
        assert same_bits(N(face)[idx], rface) and same_bits(N(t)[idx], rt) and same_bits(N(bary)[idx], rbary)
    hit = objects.trace_mesh(to, td, tv, tf, any_hit=True, accel="bvh")
    assert torch.equal(hit, face >= 0)


# ----------------------------------------------------------------------------------------------------------- shadows
@pytest.mark.parametrize("H,W,G", [(8, 16, 64), (16, 32, 48)])
def test_shadow_ratio_has_the_brute_force_bits(H, W, G):
    from pano_nerf_amd import objects
    v, f = spec.icosphere(3, RADIUS, CENTRE)
    env = gobj._hdr_probe(H, W)
    pts, nrm = gobj._floor(G)
    probe = gobj.probe_tensor(env[None], H, W)[0]
    tv, tf = T(v), T(f, torch.int32)
    want = objects.shadow_ratio(T(pts), T(nrm), probe, tv, tf, bias=1e-3)
    bvh = objects.MeshBVH.build(tv, tf)
    for accel in ("bvh", bvh):
        got = objects.shadow_ratio(T(pts), T(nrm), probe, tv, tf, bias=1e-3, accel=accel)
        assert got.shape == (G * G,) and got.dtype == torch.float32 and bits_equal(got, want)
    assert float(want.min()) < 0.5
    # non-finite points -> 1, their neighbours untouched; points above the sphere and F = 0 -> exactly 1
    p2 = pts.copy()
    p2[5, 0], p2[77, 1], p2[300, 2] = np.nan, np.inf, -np.inf
    g2 = objects.shadow_ratio(T(p2), T(nrm), probe, tv, tf, accel=bvh)
    assert bits_equal(g2, objects.shadow_ratio(T(p2), T(nrm), probe, tv, tf))
    assert np.all(N(g2)[[5, 77, 300]] == 1.0)
    up, _ = gobj._floor(G, 0.6)
    assert bool((objects.shadow_ratio(T(up), T(nrm), probe, tv, tf, accel=bvh) == 1.0).all())
    assert bool((objects.shadow_ratio(T(pts), T(nrm), probe, tv, tf[:0], accel="bvh") == 1.0).all())
    assert objects.shadow_ratio(T(pts[:0]), T(nrm[:0]), probe, tv, tf, accel=bvh).shape == (0,)
    # the number of points per launch does not show; a repeated call gives the same bits
    tp, tn = T(pts), T(nrm)
    for R in (1, 65, 1000):
        assert bits_equal(objects.shadow_ratio(tp[:R], tn[:R], probe, tv, tf, accel=bvh), want[:R]), R
    assert bits_equal(objects.shadow_ratio(tp, tn, probe.contiguous()[None], tv, tf, accel=bvh), want)


# --------------------------------------------------------------------------------------------------------- insertion
@pytest.mark.parametrize("cam", ["pano", "pinhole"])
def test_insert_object_with_a_bvh_is_insert_object(cam, monkeypatch):
    from pano_nerf_amd import objects
    model = gobj.make_model("pano", "fused_f16x2")
    camera = gobj._cameras()[cam]
    obj = gobj._object(roughness=0.4 if cam == "pinhole" else None)
    rec = Recorder(monkeypatch)
    want = objects.insert_object(model, camera, gobj.C2W, obj, probe_size=(16, 32))
    assert rec.bvh() == [] and obj._bvh is None  # the default path reaches no BVH entry point
    got = objects.insert_object(model, camera, gobj.C2W, obj, probe_size=(16, 32), accel="bvh")
    assert set(got) == set(want)
    for k in want:
        assert bits_equal(got[k], want[k]), (cam, k)
    assert float(got["mask"].sum()) > 0 and float(got["shadow"].min()) < 1
    assert rec.names.count("pn_bvh_tree") == 1 and "pn_trace_mesh_bvh" in rec.names and "pn_shadow_ratio_bvh" in rec.names
    # the object keeps its tree: a second frame builds nothing; a MeshBVH handed in is used as it is
    tree = obj._bvh
    assert isinstance(tree, objects.MeshBVH) and obj.bvh() is tree
    again = objects.insert_object(model, camera, gobj.C2W, obj, probe_size=(16, 32), accel="bvh")
    third = objects.insert_object(model, camera, gobj.C2W, obj, probe_size=(16, 32), accel=tree)
    assert rec.names.count("pn_bvh_tree") == 1
    assert all(bits_equal(again[k], want[k]) and bits_equal(third[k], want[k]) for k in want)
    # transformed() returns an object without a tree
    moved = obj.transformed(np.array([[1, 0, 0, 0.05], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]))
    assert moved._bvh is None and moved.bvh() is not tree and rec.names.count("pn_bvh_tree") == 2


def test_insert_path_builds_once(monkeypatch):
    from pano_nerf_amd import objects
    model = gobj.make_model("pano", "fused_f16x2")
    camera = gobj._cameras()["pinhole"]
    poses = np.stack([spec.look_at((0.1 + 0.05 * i, 0.05, 0.2), (0.0, 0.0, -0.6)) for i in range(3)])
    want = objects.insert_path(model, camera, poses, gobj._object(), probe_size=(8, 16), kinds=("ldr", "mask", "depth"))
    rec = Recorder(monkeypatch)
    got = objects.insert_path(model, camera, poses, gobj._object(), probe_size=(8, 16), kinds=("ldr", "mask", "depth"),
                              accel="bvh")
    assert rec.names.count("pn_bvh_tree") == 1 and rec.names.count("pn_bvh_boxes") == 1
    assert rec.names.count("pn_trace_mesh_bvh") == 3 and rec.names.count("pn_shadow_ratio_bvh") == 3
    assert "pn_trace_mesh" not in rec.names and "pn_shadow_ratio" not in rec.names
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)


def test_the_default_path_reaches_no_bvh_entry_point(monkeypatch):
    from pano_nerf_amd import objects
    rec = Recorder(monkeypatch)
    v, f = spec.icosphere(2, RADIUS, CENTRE)
    tv, tf = T(v), T(f, torch.int32)
    o, d = (T(x[:500]) for x in bspec.scene_rays(v, f))
    objects.trace_mesh(o, d, tv, tf)
    objects.trace_mesh(o, d, tv, tf, any_hit=True, accel=None)
    pts, nrm = gobj._floor(8)
    probe = gobj.probe_tensor(gobj._hdr_probe(8, 16)[None], 8, 16)[0]
    objects.shadow_ratio(T(pts), T(nrm), probe, tv, tf)
    objects.VirtualObject(tv, tf)
    assert rec.bvh() == [] and rec.names.count("pn_trace_mesh") == 2 and rec.names.count("pn_shadow_ratio") == 1
    objects.trace_mesh(o, d, tv, tf, accel="bvh")
    assert rec.bvh() == ["pn_bvh_boxes", "pn_bvh_keys", "pn_bvh_tree", "pn_trace_mesh_bvh"]


def test_the_object_cache_follows_the_mesh(monkeypatch):
    from pano_nerf_amd import objects
    v, f = spec.icosphere(2, RADIUS, CENTRE)
    obj = objects.VirtualObject(T(v), T(f, torch.int32))
    rec = Recorder(monkeypatch)
    tree = obj.bvh()
    assert obj.bvh() is tree and rec.names.count("pn_bvh_tree") == 1
    obj.vertices += 0.25  # in place: the kept tree no longer fits
    moved = obj.bvh()
    assert moved is not tree and obj.bvh() is moved and rec.names.count("pn_bvh_tree") == 2
    fresh = objects.MeshBVH.build(obj.vertices, obj.faces)
    assert bits_equal(moved.nodes, fresh.nodes) and bits_equal(moved.tris, fresh.tris)
    obj.faces = obj.faces[:100].contiguous()  # another tensor
    assert obj.bvh().F == 100
