"""The sparse radiance volume without a GPU: the numpy restatement of its layout (tests/_sparse_ref.py) held to the facts
the header states, the exactness argument of DESIGN.md 6p run on the restated marcher (tests/_volume_ref.py), the cap on
fragile rays for the fp16-rounded scenes, and the file format."""
import functools
import json

import numpy as np
import pytest

import _sparse_ref as sref
import _sparse_scenes as scenes
import _volume_ref as ref


@functools.lru_cache(maxsize=None)
def packed(name, half=False):
    table, pool = sref.pack(scenes.volume(name)[0], np.float16 if half else np.float32)
    return table, pool


def march(name, data, t_min=1e-3, big=False, occ=None, jumps=False):
    _, bounds, deg, _ = scenes.volume(name)
    lo, step = scenes.placement(bounds, data.shape[:3])
    ms = scenes.big_step(name) if big else scenes.march_step(bounds, data.shape[:3])
    r = scenes.rays(name)
    return ref.march(data, lo, step, deg, r["origins"], r["directions"], r["near"], r["far"], ms, t_min, occ, jumps)


def vertex_mask(table, res):
    """bool [nx, ny, nz]: the vertices of present bricks, shared faces included"""
    mask = np.zeros(res, bool)
    for _, grid, _ in sref._blocks(table, res):
        mask[grid] = True
    return mask


@pytest.mark.parametrize("name", scenes.NAMES)
def test_pack_then_unpack_is_the_identity_on_present_bricks(name):
    data = scenes.volume(name)[0]
    table, pool = packed(name)
    assert pool.dtype == np.float32 and pool.shape[1:] == (9, 9, 9, data.shape[3])
    back = sref.unpack(table, pool, data.shape[:3])
    mask = vertex_mask(table, data.shape[:3])
    assert np.array_equal(back[mask].view(np.uint32), data[mask].view(np.uint32))
    assert not back[~mask].view(np.uint32).any()
    with np.errstate(invalid="ignore"):
        assert not (data[~mask][:, 0] > 0).any()  # nothing positive is left out


@pytest.mark.parametrize("name", scenes.NAMES)
def test_slots_ascend_with_the_brick_index(name):
    data = scenes.volume(name)[0]
    table, pool = packed(name)
    occ = ref.occupancy(data)
    assert table.dtype == np.int32 and table.shape == occ.shape
    assert np.array_equal(table >= 0, occ > 0)
    assert np.array_equal(table.reshape(-1)[table.reshape(-1) >= 0], np.arange(pool.shape[0]))


def test_known_tables():
    assert packed("corner")[1].shape[0] == 8 and (packed("corner")[0] >= 0).all()
    assert np.array_equal(packed("gap")[0][:, :, 0], [[0, 1], [-1, -1], [2, 3]])
    assert np.array_equal(packed("tiny16")[0].reshape(-1), [0, 1])
    assert np.array_equal(packed("single")[0].reshape(-1), [-1] * 7 + [0])


@pytest.mark.parametrize("name", scenes.NAMES)
def test_apron_copies_agree_and_partial_bricks_pad_with_zeros(name):
    data = scenes.volume(name)[0]
    res = data.shape[:3]
    table, pool = packed(name)
    bits = pool.view(np.uint32)
    nb = table.shape
    shared = 0
    for (bi, bj, bk), slot in np.ndenumerate(table):
        if slot < 0:
            continue
        n = [min(8 * b + 9, r) - 8 * b for b, r in zip((bi, bj, bk), res)]
        full = np.zeros((9, 9, 9), bool)
        full[:n[0], :n[1], :n[2]] = True
        assert not bits[slot][~full].any()
        for axis, b in enumerate((bi, bj, bk)):  # the far face of this brick is the near face of the next one
            nxt = [bi, bj, bk]
            nxt[axis] += 1
            if nxt[axis] < nb[axis] and table[tuple(nxt)] >= 0:
                far = np.take(bits[slot], 8, axis=axis)
                near = np.take(bits[table[tuple(nxt)]], 0, axis=axis)
                assert np.array_equal(far, near), (name, (bi, bj, bk), axis)
                shared += 1
    if name == "corner":
        assert shared == 12
        copies = [pool[table[bi, bj, bk], 8 - 8 * bi, 8 - 8 * bj, 8 - 8 * bk] for bi in (0, 1) for bj in (0, 1) for bk in (0, 1)]
        assert all(np.array_equal(c, data[8, 8, 8]) for c in copies) and copies[0][0] == 40.0


@pytest.mark.parametrize("name", scenes.NAMES)
def test_marching_the_expansion_is_marching_the_volume(name):
    """the exactness argument: zeroing the vertices of absent bricks changes no output and no tap count"""
    data = scenes.volume(name)[0]
    table, pool = packed(name)
    back = sref.unpack(table, pool, data.shape[:3])
    assert np.array_equal(ref.occupancy(back), ref.occupancy(data))
    for t_min, big in ((1e-3, False), (0.0, True)):
        want, got = march(name, data, t_min, big), march(name, back, t_min, big)
        for k in ("rgb", "depth", "acc", "attrs", "marched", "evaluated", "hits"):
            assert np.array_equal(want[k], got[k], equal_nan=True), (name, t_min, big, k)


def test_gap_rays_cross_the_absent_brick():
    data = scenes.volume("gap")[0]
    occ = ref.occupancy(data)
    n_base = scenes.base.rays()["near"].shape[0]
    plain, jumped = march("gap", data, 0.0), march("gap", data, 0.0, occ=occ, jumps=True)  # t_min 0: no ray stops early
    for k in ("rgb", "depth", "acc"):
        assert np.array_equal(plain[k], jumped[k])
    extra = slice(n_base, None)
    assert plain["marched"][extra].all() and (plain["hits"][extra] > 0).all()
    assert (jumped["evaluated"][extra] < plain["evaluated"][extra]).all()  # every added ray skips samples of the gap


@pytest.mark.parametrize("name", scenes.NAMES)
def test_fp16_rounded_scenes_keep_fragile_rays_under_the_cap(name):
    data = scenes.half_volume(name)[0]
    for t_min in (0.0, 1e-3, 0.5):
        got = march(name, data, t_min)
        assert got["fragile"].mean() <= 0.01, (name, t_min, int(got["fragile"].sum()))
    assert march(name, data, 0.0, True)["fragile"].mean() <= 0.01
    assert march(name, scenes.volume(name)[0], 1e-3)["fragile"].mean() <= 0.01  # the three new scenes in fp32 too
    # jumping over the ORIGINAL occupancy (what the sparse fp16 volume does) equals the plain loop on the rounded data
    occ = ref.occupancy(scenes.volume(name)[0])
    plain, jumped = march(name, data), march(name, data, occ=occ, jumps=True)
    for k in ("rgb", "depth", "acc", "attrs"):
        assert np.array_equal(plain[k], jumped[k], equal_nan=True), (name, k)


def test_fp16_rounding_of_tiny16_is_ieee():
    data, half = scenes.volume("tiny16")[0], scenes.half_volume("tiny16")[0]
    sub = 2.0 ** -24  # the smallest half subnormal
    assert half[1, 1, 1, 0] == 17 * sub and half[1, 1, 2, 0] == sub and half[1, 1, 3, 0] == 0
    assert half[1, 2, 1, 0] == 65504 and half[1, 2, 2, 0] == 1 and half[1, 2, 3, 0] == 1 + 2.0 ** -9
    assert half[1, 3, 1, 0] == 0 and half[9, 4, 4, 0] == 0 and data[9, 4, 4, 0] > 0
    assert np.array_equal(half[2, 2, 1, 1:], np.float32([-0.0, 2.0 ** -14, 1007 * sub])) and np.signbit(half[2, 2, 1, 1])
    assert np.isfinite(half).all()
    # brick (1, 0, 0) is present in the sparse form and unoccupied in its fp16 expansion
    assert ref.occupancy(data).reshape(-1).tolist() == [1, 1] and ref.occupancy(half).reshape(-1).tolist() == [1, 0]
    _, pool = packed("tiny16", True)
    assert pool.dtype == np.float16 and pool.shape[0] == 2 and not pool[1, ..., 0].astype(np.float32).max() > 0


@pytest.mark.parametrize("half", [False, True])
def test_files_round_trip_bit_for_bit(tmp_path, half):
    from pano_nerf_amd import volume
    for name in ("nan", "tiny16", "gap"):
        data, bounds, deg, attrs = scenes.volume(name)
        table, pool = packed(name, half)
        path = str(tmp_path / name)
        volume.write_sparse_volume_files(path, table, pool, bounds, data.shape[:3], deg, attrs)
        t2, p2, b2, r2, d2, a2 = volume.read_sparse_volume_files(path)
        assert t2.dtype == np.int32 and np.array_equal(t2, table)
        assert p2.dtype == pool.dtype and p2.shape == pool.shape
        assert np.array_equal(p2.view(np.uint16 if half else np.uint32), pool.view(np.uint16 if half else np.uint32))
        assert (b2, r2, d2, a2) == (bounds, data.shape[:3], deg, attrs)
        meta = json.load(open(tmp_path / name / "volume.json"))
        assert meta["format"] == "pano_nerf_amd.sparse_radiance_volume" and meta["version"] == 1
        assert meta["bricks"] == pool.shape[0] and meta["channels"] == data.shape[3]
        assert meta["dtype"] == ("<f2" if half else "<f4") and meta["resolution"] == list(data.shape[:3])


def test_an_empty_pool_round_trips(tmp_path):
    from pano_nerf_amd import volume
    table = np.full((2, 1, 1), -1, np.int32)
    pool = np.zeros((0, 9, 9, 9, 4), np.float16)
    volume.write_sparse_volume_files(str(tmp_path / "e"), table, pool, scenes.BOUNDS, (10, 9, 9), 0, ())
    t2, p2, _, r2, _, _ = volume.read_sparse_volume_files(str(tmp_path / "e"))
    assert np.array_equal(t2, table) and p2.shape == pool.shape and p2.dtype == np.float16 and r2 == (10, 9, 9)


def test_bad_files_are_rejected_by_name(tmp_path):
    from pano_nerf_amd import volume
    data, bounds, deg, attrs = scenes.volume("gap")
    table, pool = packed("gap")
    path = tmp_path / "v"
    write = lambda: volume.write_sparse_volume_files(str(path), table, pool, bounds, data.shape[:3], deg, attrs)

    def edit(**fields):
        meta = json.load(open(path / "volume.json"))
        meta.update(fields)
        json.dump(meta, open(path / "volume.json", "w"))

    write()
    with pytest.raises(ValueError, match="not a radiance volume"):
        volume.read_volume_files(str(path))  # the dense reader keeps rejecting what is not its own
    edit(format="pano_nerf_amd.radiance_volume")
    with pytest.raises(ValueError, match="not a sparse radiance volume"):
        volume.read_sparse_volume_files(str(path))
    write()
    edit(version=2)
    with pytest.raises(ValueError, match="version 2"):
        volume.read_sparse_volume_files(str(path))
    write()
    with open(path / "pool.bin", "ab") as fh:
        fh.write(b"\0\0\0\0")
    with pytest.raises(ValueError, match="pool.bin"):
        volume.read_sparse_volume_files(str(path))
    write()
    with open(path / "table.bin", "wb") as fh:
        fh.write(table.tobytes()[:-4])
    with pytest.raises(ValueError, match="table.bin"):
        volume.read_sparse_volume_files(str(path))
    write()
    edit(dtype="<f8")
    with pytest.raises(ValueError, match="dtype"):
        volume.read_sparse_volume_files(str(path))
    with pytest.raises(ValueError, match="table"):
        volume.write_sparse_volume_files(str(tmp_path / "w"), table[:2], pool, bounds, data.shape[:3], deg, attrs)
    with pytest.raises(ValueError, match="pool"):
        volume.write_sparse_volume_files(str(tmp_path / "w"), table, pool[..., :3], bounds, data.shape[:3], deg, attrs)
    with pytest.raises(ValueError, match="present"):
        volume.write_sparse_volume_files(str(tmp_path / "w"), table, pool[:2], bounds, data.shape[:3], deg, attrs)
    dense = tmp_path / "d"
    volume.write_volume_files(str(dense), data, bounds, deg, attrs)
    with pytest.raises(ValueError, match="not a sparse radiance volume"):
        volume.read_sparse_volume_files(str(dense))
