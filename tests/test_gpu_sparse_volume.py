"""The sparse radiance volume on the device: pn_volume_pack / pn_volume_unpack against the numpy restatement of the layout
(tests/_sparse_ref.py) bit for bit, pn_volume_march_sparse against pn_volume_march on the dense expansion bit for bit
(taps included for fp32 storage), against the fp64 restatement of the marcher to ONE fp32 ulp, the wrappers, the sparse
bake, the files and the error paths.

Tolerances: none of their own.  Sparse against dense is exact (the same fp64 arithmetic on the same stored values).
Against the restatement it is tests/test_gpu_volume.py's rule, restated here: one fp32 ulp plus 2^-40 of the sum of
absolute terms, fragile rows left out under the 1 % cap tests/test_sparse_volume_cpu.py holds for these scenes."""
import functools

import numpy as np
import pytest
import torch

import _sparse_ref as sref
import _sparse_scenes as scenes
import _volume_ref as ref

pytestmark = pytest.mark.gpu

SLACK = 2.0 ** -40
SHAPE, NULL = -1, -3  # PN_ERR_BAD_SHAPE, PN_ERR_NULL
DTYPES = {False: torch.float32, True: torch.float16}


def dev():
    return torch.device("cuda:0")


def on_dev(a):
    return torch.from_numpy(np.array(a)).to(dev())


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@functools.lru_cache(maxsize=None)
def dense(name):
    from pano_nerf_amd import volume
    data, bounds, deg, attrs = scenes.volume(name)
    return volume.RadianceVolume(on_dev(data.copy()), bounds, deg, attrs)


@functools.lru_cache(maxsize=None)
def sparse(name, half=False):
    return dense(name).to_sparse(DTYPES[half])


@functools.lru_cache(maxsize=None)
def expanded(name, half):
    """the dense expansion of the fp16 volume (for fp32 storage it marches like dense(name) itself)"""
    return sparse(name, half).to_dense()


@functools.lru_cache(maxsize=None)
def device_rays(name):
    return {k: on_dev(v) for k, v in scenes.rays(name).items()}


@functools.lru_cache(maxsize=None)
def host_pack(name, half):
    return sref.pack(scenes.volume(name)[0], np.float16 if half else np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, half, t_min, big):
    """the restated marcher on the restated expansion of the restated pool"""
    data, bounds, deg, _ = scenes.volume(name)
    table, pool = host_pack(name, half)
    lo, step = scenes.placement(bounds, data.shape[:3])
    ms = scenes.big_step(name) if big else scenes.march_step(bounds, data.shape[:3])
    r = scenes.rays(name)
    return ref.march(sref.unpack(table, pool, data.shape[:3]), lo, step, deg, r["origins"], r["directions"], r["near"],
                     r["far"], ms, t_min)


def march(vol, name, step=None, t_min=1e-3, skip=True, outputs=None):
    from pano_nerf_amd import volume
    r = device_rays(name)
    outputs = ("rgb", "depth", "acc") + vol.attribute_names + ("taps",) if outputs is None else outputs
    return volume.march_rays(vol, r["origins"], r["directions"], r["near"], r["far"], step, t_min, skip, outputs)


def same_bits(got, want, what, skip_keys=()):
    assert set(got) == set(want)
    for k in got:
        if k not in skip_keys:
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (what, k)


def compare(got, want, what):
    """tests/test_gpu_volume.py's compare: every output against the restatement; returns the worst ulp"""
    keep = ~want["fragile"]
    assert keep.mean() >= 0.99 or keep.size < 100, (what, int((~keep).sum()))
    worst = 0.0
    names = [k for k in got if k not in ("rgb", "depth", "acc", "taps")]
    pairs = [("rgb", got["rgb"], want["rgb"], want["abs_rgb"]), ("acc", got["acc"][:, 0], want["acc"], want["acc"]),
             ("depth", got["depth"][:, 0], want["depth"], want["abs_wt"] * 0.0)]
    if names:
        pairs.append(("attrs", torch.cat([got[k] for k in names], 1), want["attrs"], want["abs_attrs"]))
    for name, g, w, a in pairs:
        g, w, a = g.cpu().numpy()[keep], w[keep], a[keep]
        assert np.array_equal(g == 0, w.astype(np.float32) == 0), (what, name, "zero outputs differ")
        u = ref.ulps(g, w, SLACK * a)
        worst = max(worst, float(u.max()) if u.size else 0.0)
        assert (u <= 1.0).all(), (what, name, float(u.max()))
    dead = ~want["marched"]
    for k, v in got.items():
        assert not v.cpu().numpy()[dead].any(), (what, k, "an invalid row wrote something")
    return worst


# ------------------------------------------------------------------------------------------------ 1. pack and unpack
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("name", scenes.NAMES)
def test_pack_and_unpack_match_the_restatement(name, half):
    data = scenes.volume(name)[0]
    table, pool = host_pack(name, half)
    sp = sparse(name, half)
    assert sp.table.dtype == torch.int32 and sp.dtype == DTYPES[half] and sp.bricks == pool.shape[0]
    assert sp.resolution == data.shape[:3] and sp.channels == data.shape[3]
    assert torch.equal(sp.table, on_dev(table))
    assert sp.pool.shape == pool.shape and torch.equal(bits(sp.pool), bits(on_dev(pool)))
    assert torch.equal(sp.occupancy, dense(name).occupancy)
    assert sp.dense_nbytes == data.nbytes and sp.nbytes == table.nbytes + pool.nbytes
    back = sp.to_dense()
    assert torch.equal(bits(back.data), bits(on_dev(sref.unpack(table, pool, data.shape[:3]))))
    assert back.bounds == sp.bounds and back.sh_degree == sp.sh_degree and back.attribute_names == sp.attribute_names


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("name", scenes.NAMES)
def test_pack_from_rows_matches_the_restatement(name, half):
    """rows mode: the kept vertices in a shuffled order behind a vertex -> row map; a vertex without a row packs as 0"""
    from pano_nerf_amd import _lib
    data = scenes.volume(name)[0]
    res, C = data.shape[:3], data.shape[3]
    N = res[0] * res[1] * res[2]
    i, j, k = np.meshgrid(*[np.arange(n) for n in res], indexing="ij")
    with np.errstate(invalid="ignore"):
        drop = ~(data[..., 0] > 0) & ((i + j + k) % 3 == 0)  # never a positive vertex: the table stays the volume's
    zeroed = np.where(drop[..., None], np.float32(0), data)
    table, want = sref.pack(zeroed, np.float16 if half else np.float32, host_pack(name, half)[0])
    order = np.random.default_rng(7).permutation(np.flatnonzero(~drop.reshape(-1)))
    rows = np.ascontiguousarray(data.reshape(N, C)[order])
    vertex_row = np.full(N, -1, np.int32)
    vertex_row[order] = np.arange(order.size, dtype=np.int32)
    B = want.shape[0]
    t_d, r_d, v_d = on_dev(table), on_dev(rows), on_dev(vertex_row)
    pool = torch.full(want.shape, 7.0, dtype=DTYPES[half], device=dev())
    _lib.call("pn_volume_pack", *res, C, t_d.data_ptr(), B, None, r_d.data_ptr(), order.size, v_d.data_ptr(), int(half),
              pool.data_ptr(), _lib.stream(dev()))
    assert torch.equal(bits(pool), bits(on_dev(want)))


# --------------------------------------------------------------------------------- 2. sparse against dense, bit for bit
@pytest.mark.parametrize("name", scenes.NAMES)
def test_sparse_march_is_the_dense_march_bit_for_bit(name):
    vol, sp = dense(name), sparse(name)
    for step in (None, float(scenes.big_step(name))):
        for t_min in (0.0, 1e-3, 0.5):
            for skip in (True, False):
                same_bits(march(sp, name, step, t_min, skip), march(vol, name, step, t_min, skip), (name, step, t_min, skip))


@pytest.mark.parametrize("name", scenes.NAMES)
def test_fp16_march_is_the_march_of_its_expansion(name):
    sp, vol = sparse(name, True), expanded(name, True)
    for step in (None, float(scenes.big_step(name))):
        for t_min in (0.0, 1e-3, 0.5):
            for skip in (True, False):
                same_bits(march(sp, name, step, t_min, skip), march(vol, name, step, t_min, skip), (name, step, t_min, skip),
                          skip_keys=("taps",))


def test_taps_of_an_absent_brick():
    """skip off: a sample in an absent brick is one sigma tap; skip on: the jump saves them.  fp16: the brick of tiny16
    whose only positive sigma rounds to 0 stays present, so the expansion (which skips it) takes fewer sigma taps."""
    plain, jumped = march(sparse("gap"), "gap", None, 0.0, False)["taps"], march(sparse("gap"), "gap", None, 0.0, True)["taps"]
    assert torch.equal(plain[:, 1], jumped[:, 1]) and bool((jumped[:, 0] <= plain[:, 0]).all())
    extra = slice(scenes.base.rays()["near"].shape[0], None)
    assert bool((jumped[extra, 0] < plain[extra, 0]).all()) and bool((plain[extra, 1] > 0).all())
    a, b = march(sparse("tiny16", True), "tiny16")["taps"], march(expanded("tiny16", True), "tiny16")["taps"]
    assert torch.equal(a[:, 1], b[:, 1]) and bool((a[:, 0] >= b[:, 0]).all()) and int(a[:, 0].sum()) > int(b[:, 0].sum())


# -------------------------------------------------------------------------------------- 3. against the restatement
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("name", scenes.NAMES)
def test_sparse_march_matches_the_restatement(name, half):
    sp = sparse(name, half)
    outs = ("rgb", "depth", "acc") + sp.attribute_names
    worst = 0.0
    for t_min in (0.0, 1e-3, 0.5):
        for big in (False, True):
            want = reference(name, half, t_min, big)
            for skip in (True, False):
                got = march(sp, name, float(scenes.big_step(name)) if big else None, t_min, skip, outs)
                worst = max(worst, compare(got, want, (name, half, t_min, big, skip)))
    print(f"{name} {'fp16' if half else 'fp32'}: worst ulp {worst:.3f}")


# ----------------------------------------------------------------------------------------------------- 4. wrappers
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("camera", ["pinhole", "fisheye"])
def test_render_volume_takes_a_sparse_volume(camera, half):
    from pano_nerf_amd import views, volume
    ctor, args = scenes.base.CAMERAS[camera]
    cam = getattr(views, ctor)(*args)
    pose = scenes.base.camera_pose()
    sp, vol = sparse("checker", half), (expanded("checker", True) if half else dense("checker"))
    outs = ("rgb", "depth", "acc") + sp.attribute_names
    a = volume.render_volume(sp, cam, pose, outs, scenes.base.CAMERA_NEAR, scenes.base.CAMERA_FAR)
    b = volume.render_volume(vol, cam, pose, outs, scenes.base.CAMERA_NEAR, scenes.base.CAMERA_FAR)
    for k in outs:
        assert a[k].shape == b[k].shape and torch.equal(bits(a[k].contiguous()), bits(b[k].contiguous())), (camera, k)
    assert float(a["acc"].max()) > 0.5
    if camera == "fisheye":
        mask = on_dev(views.camera_mask(cam))
        assert not bool(mask.all()) and not a["acc"][0, 0][~mask.reshape(cam.h, cam.w)].any()


def test_probes_and_paths_take_a_sparse_volume():
    from pano_nerf_amd import views, volume
    pos = on_dev(np.array([[0.013, -0.021, 0.037], [0.3, 0.2, -0.9]], np.float32))
    a = volume.volume_probes(sparse("partial"), pos, 8, 16, 0.0, 2.5)
    assert a.shape == (2, 3, 8, 16) and float(a.max()) > 0
    assert torch.equal(a, volume.volume_probes(dense("partial"), pos, 8, 16, 0.0, 2.5))
    cam = views.perspective_camera(12, 16, 14.0)
    poses = np.stack([scenes.base.camera_pose()] * 2)
    poses[1, :3, 3] += (0.05, 0.02, -0.03)
    kinds = ("ldr", "depth", "albedo")
    fa = volume.render_volume_path(sparse("checker"), cam, poses, kinds, scenes.base.CAMERA_NEAR, scenes.base.CAMERA_FAR)
    fb = volume.render_volume_path(dense("checker"), cam, poses, kinds, scenes.base.CAMERA_NEAR, scenes.base.CAMERA_FAR)
    for k in kinds:
        assert torch.equal(fa[k], fb[k]), k
    with pytest.raises(ValueError):
        volume.render_volume_path(sparse("gap"), cam, poses, ("albedo",))  # the volume has no albedo


# --------------------------------------------------------------------------------------------------------- 5. bake
def make_model():
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    m = pn.PanoMipNeRF(num_samples=8, rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    m.mlp.load_state_dict(orc.init_params(4, 5))
    return m.to(dev())


def test_sparse_bake_is_the_dense_bake():
    from pano_nerf_amd import geometry, volume
    model = make_model()
    bounds, res = ((-0.8, -0.6, -0.7), (0.7, 0.9, 0.6)), (10, 9, 17)
    sigma = geometry.density_grid(model, bounds, res).cpu().numpy()
    # the largest sigma of each of the 2 x 1 x 2 bricks (shared faces included); a threshold between the two smallest
    # distinct ones drops at least one brick and keeps at least one
    tops = sorted({float(sigma[8 * bi:8 * bi + 9, :, 8 * bk:8 * bk + 9].max()) for bi in (0, 1) for bk in (0, 1)})
    assert len(tops) >= 2
    sigma_min = 0.5 * (tops[0] + tops[1])
    vol = volume.bake_volume(model, bounds, res, sigma_min=sigma_min)
    sp = volume.bake_volume(model, bounds, res, sigma_min=sigma_min, sparse=True)
    assert isinstance(sp, volume.SparseRadianceVolume) and sp.dtype == torch.float32 and 0 < sp.bricks < 4
    assert sp.attribute_names == vol.attribute_names and sp.sh_degree == vol.sh_degree and sp.bounds == vol.bounds
    assert torch.equal(bits(sp.to_dense().data), bits(vol.data))
    packed = vol.to_sparse()
    assert torch.equal(sp.table, packed.table) and torch.equal(bits(sp.pool), bits(packed.pool))
    assert float((vol.sigma > 0).float().mean()) > 0  # something survived, and pruned vertices are in the pool as 0
    sp16 = volume.bake_volume(model, bounds, res, sigma_min=sigma_min, sparse=True, dtype=torch.float16)
    packed16 = vol.to_sparse(torch.float16)
    assert sp16.dtype == torch.float16 and torch.equal(sp16.table, packed16.table)
    assert torch.equal(bits(sp16.pool), bits(packed16.pool))
    # nothing survives: an empty pool marches to nothing and expands to zeros
    empty = volume.bake_volume(model, bounds, res, sigma_min=float(sigma.max()), sparse=True, dtype=torch.float16)
    assert empty.bricks == 0 and empty.pool.shape == (0, 9, 9, 9, empty.channels) and not bool(empty.occupancy.any())
    zeros = empty.to_dense()
    assert not bool(zeros.data.any())
    r = device_rays("gap")
    for skip in (True, False):
        a = volume.march_rays(empty, r["origins"], r["directions"], r["near"], r["far"], skip=skip, outputs=("rgb", "acc", "depth"))
        b = volume.march_rays(zeros, r["origins"], r["directions"], r["near"], r["far"], skip=skip, outputs=("rgb", "acc", "depth"))
        assert not bool(a["rgb"].any()) and not bool(a["acc"].any()) and torch.equal(a["depth"], b["depth"])
    with pytest.raises(ValueError, match="float32 or torch.float16"):
        volume.bake_volume(model, bounds, res, sparse=True, dtype=torch.bfloat16)


# -------------------------------------------------------------------------------------------------------- 6. files
@pytest.mark.parametrize("half", [False, True])
def test_save_and_load_bit_for_bit(tmp_path, half):
    from pano_nerf_amd import volume
    for name in ("nan", "tiny16"):
        sp = sparse(name, half)
        sp.save(str(tmp_path / name))
        for back in (volume.SparseRadianceVolume.load(str(tmp_path / name), dev()), volume.load_volume(str(tmp_path / name), dev())):
            assert isinstance(back, volume.SparseRadianceVolume) and back.dtype == sp.dtype
            assert torch.equal(back.table, sp.table) and torch.equal(bits(back.pool), bits(sp.pool))
            assert back.bounds == sp.bounds and back.lo == sp.lo and back.step == sp.step
            assert back.resolution == sp.resolution and back.sh_degree == sp.sh_degree
            assert back.attribute_names == sp.attribute_names
    dense("nan").save(str(tmp_path / "dense"))
    back = volume.load_volume(str(tmp_path / "dense"), dev())
    assert isinstance(back, volume.RadianceVolume) and torch.equal(bits(back.data), bits(dense("nan").data))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        volume.load_volume(str(tmp_path / "nan"), "cpu")


# ------------------------------------------------------------------------------------------------- 7. fp16 overflow
def test_fp16_overflow_raises_only_in_a_present_brick():
    from pano_nerf_amd import volume
    data, bounds, deg, attrs = scenes.volume("gap")
    bad = data.copy()
    bad[3, 3, 3, 2] = 1e5  # brick (0, 0, 0) is present
    with pytest.raises(ValueError, match=r"coeff\[0\]\[g\]"):
        volume.RadianceVolume(on_dev(bad), bounds, deg, attrs).to_sparse(torch.float16)
    volume.RadianceVolume(on_dev(bad), bounds, deg, attrs).to_sparse(torch.float32)
    fine = data.copy()
    fine[12, 3, 3, 2] = 1e5   # strictly inside the absent brick (1, 0, 0)
    fine[3, 3, 3, 5] = np.inf  # an infinity of the source is not an overflow
    sp = volume.SparseRadianceVolume.from_dense(volume.RadianceVolume(on_dev(fine), bounds, deg, attrs), torch.float16)
    assert sp.bricks == 4 and bool(torch.isinf(sp.pool).any())
    with pytest.raises(ValueError, match="float32 or torch.float16"):
        dense("gap").to_sparse(torch.float64)


# --------------------------------------------------------------------------------------------------- 8. error paths
def test_entry_point_argument_errors():
    from pano_nerf_amd import _lib
    lib = _lib.load()
    sp = sparse("gap")
    res, C, B = sp.resolution, sp.channels, sp.bricks
    t, p, s = sp.table.data_ptr(), sp.pool.data_ptr(), _lib.stream(dev())
    d = dense("gap").data.data_ptr()
    out = torch.empty(*res, C, device=dev()).data_ptr()
    vr = torch.full((res[0] * res[1] * res[2],), -1, dtype=torch.int32, device=dev()).data_ptr()
    pack = lambda *a: lib.pn_volume_pack(*a, s)
    assert pack(*res, C, None, B, d, None, 0, None, 0, p) == NULL            # no table
    assert pack(*res, C, t, B, None, None, 0, None, 0, p) == NULL            # no source
    assert pack(*res, C, t, B, d, None, 0, None, 0, None) == NULL            # no pool
    assert pack(*res, C, t, B, None, d, 5, None, 0, p) == NULL               # rows without a vertex map
    assert pack(*res, C, t, B, d, d, 5, vr, 0, p) == SHAPE                   # both sources
    assert pack(*res, C, t, -1, d, None, 0, None, 0, p) == SHAPE             # B < 0
    assert pack(*res, C, t, 7, d, None, 0, None, 0, p) == SHAPE              # more slots than the table has bricks
    assert pack(1, res[1], res[2], C, t, B, d, None, 0, None, 0, p) == SHAPE  # an axis with one vertex
    assert pack(*res, 0, t, B, d, None, 0, None, 0, p) == SHAPE
    assert pack(*res, C, t, B, None, None, -1, vr, 0, p) == SHAPE            # M < 0
    assert pack(*res, C, t, 0, d, None, 0, None, 0, None) == 0               # an empty pool: nothing to launch
    unpack = lambda *a: lib.pn_volume_unpack(*a, s)
    assert unpack(*res, C, None, B, p, 0, out) == NULL
    assert unpack(*res, C, t, B, None, 0, out) == NULL
    assert unpack(*res, C, t, B, p, 0, None) == NULL
    assert unpack(*res, C, t, 7, p, 0, out) == SHAPE
    assert unpack(*res, C, t, -2, p, 0, out) == SHAPE
    assert unpack(res[0], 1, res[2], C, t, B, p, 0, out) == SHAPE
    assert unpack(2048, 2048, 2048, C, t, B, p, 0, out) == SHAPE             # 2^33 vertices
    r = device_rays("gap")
    R = r["near"].shape[0]
    rays = [r[k].data_ptr() for k in ("origins", "directions", "near", "far")]
    rgb = torch.empty(R, 3, device=dev()).data_ptr()
    tail = (rgb, None, None, None, None, s)
    grid = (*sp.lo, *sp.step)
    msp = lib.pn_volume_march_sparse
    assert msp(R, *res, 1, 0, None, p, 0, 1, *grid, *rays, 0.02, 1e-3, *tail) == NULL
    assert msp(R, *res, 1, 0, t, p, 0, 1, *grid, None, *rays[1:], 0.02, 1e-3, *tail) == NULL
    assert msp(R, *res, 3, 0, t, p, 0, 1, *grid, *rays, 0.02, 1e-3, *tail) == SHAPE
    assert msp(R, *res, 1, 9, t, p, 0, 1, *grid, *rays, 0.02, 1e-3, *tail) == SHAPE
    assert msp(R, res[0], res[1], 1, 1, 0, t, p, 0, 1, *grid, *rays, 0.02, 1e-3, *tail) == SHAPE
    assert msp(R, *res, 1, 0, t, p, 0, 1, *grid, *rays, 0.0, 1e-3, *tail) == SHAPE
    assert msp(R, *res, 1, 0, t, p, 0, 1, *grid, *rays, 0.02, -1.0, *tail) == SHAPE
    assert msp(-1, *res, 1, 0, t, p, 0, 1, *grid, *rays, 0.02, 1e-3, *tail) == SHAPE
    assert msp(0, *res, 1, 0, None, None, 0, 1, *grid, None, None, None, None, 0.02, 1e-3, *tail) == 0  # R = 0 launches nothing
    torch.cuda.synchronize()


def test_constructor_errors():
    from pano_nerf_amd import volume
    sp = sparse("gap")
    args = (sp.bounds, sp.resolution, sp.sh_degree, sp._attrs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        volume.SparseRadianceVolume(sp.table.cpu(), sp.pool, *args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        volume.SparseRadianceVolume(sp.table, sp.pool.cpu(), *args)
    with pytest.raises(ValueError, match="table"):
        volume.SparseRadianceVolume(sp.table.to(torch.int64), sp.pool, *args)
    with pytest.raises(ValueError, match="table"):
        volume.SparseRadianceVolume(sp.table[:2].contiguous(), sp.pool, *args)
    with pytest.raises(ValueError, match="pool"):
        volume.SparseRadianceVolume(sp.table, sp.pool[..., :3].contiguous(), *args)
    with pytest.raises(ValueError, match="contiguous"):
        volume.SparseRadianceVolume(sp.table, sp.pool.to(torch.float64), *args)
    with pytest.raises(ValueError, match="slots"):
        volume.SparseRadianceVolume(sp.table, sp.pool[:3].contiguous(), *args)  # B inconsistent with the table
    with pytest.raises(ValueError, match="slots"):
        volume.SparseRadianceVolume(sp.table.flip(0).contiguous(), sp.pool, *args)  # slots that do not ascend
    with pytest.raises(ValueError, match="slots"):
        volume.SparseRadianceVolume(torch.full_like(sp.table, -2), sp.pool[:0].contiguous(), *args)
    with pytest.raises(ValueError, match="RadianceVolume"):
        volume.SparseRadianceVolume.from_dense(sp)
    with pytest.raises(ValueError, match="SparseRadianceVolume"):
        volume.march_rays(object(), None, None, 0.0, 1.0)
    again = volume.SparseRadianceVolume(sp.table, sp.pool, *args)
    assert again.bricks == 4 and again.lo == sp.lo and again.step == sp.step
