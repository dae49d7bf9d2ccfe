"""Host side of the texture-mapped materials: the PNG reader, the OBJ / MTL reader, and the sanity of the numpy reference
(tests/_textures_ref.py) on cases worked out by hand.  No GPU."""
import math
import os
import struct
import zlib

import numpy as np
import pytest

import _textures_ref as ref


# ------------------------------------------------------------------------------------------------------ read_png
def _chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xffffffff)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def _filter_rows(img, ftype):
    """the PNG filter of every row of img [H, W, C] uint8, by the specification's formulas (byte by byte)"""
    h, w, c = img.shape
    flat = img.reshape(h, w * c).astype(np.int64)
    out = b""
    for y in range(h):
        ft = ftype if ftype is not None else y % 5
        row = bytearray([ft])
        for i in range(w * c):
            a = int(flat[y, i - c]) if i >= c else 0
            b = int(flat[y - 1, i]) if y else 0
            cc = int(flat[y - 1, i - c]) if (y and i >= c) else 0
            pred = (0, a, b, (a + b) // 2, _paeth(a, b, cc))[ft]
            row.append((int(flat[y, i]) - pred) & 255)
        out += bytes(row)
    return out


def _png(img, ftype, depth=8, ctype=None, interlace=0, idat_split=None):
    img = img if img.ndim == 3 else img[:, :, None]
    h, w, c = img.shape
    ctype = {1: 0, 2: 4, 3: 2, 4: 6}[c] if ctype is None else ctype
    z = zlib.compress(_filter_rows(img, ftype), 6)
    parts = [z] if not idat_split else [z[i:i + idat_split] for i in range(0, len(z), idat_split)]
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace)) +
            _chunk(b"gAMA", struct.pack(">I", 45455)) + b"".join(_chunk(b"IDAT", p) for p in parts) + _chunk(b"IEND", b""))


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("ftype", [0, 1, 2, 3, 4, None])
def test_read_png_every_filter_and_colour_type(tmp_path, ftype, channels):
    from pano_nerf_amd import io_exr
    rng = np.random.default_rng(10 * channels + (ftype or 7))
    for h, w in ((3, 5), (1, 1), (7, 2)):
        img = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
        path = str(tmp_path / f"f{h}x{w}.png")
        with open(path, "wb") as f:
            f.write(_png(img, ftype))
        got = io_exr.read_png(path)
        assert got.dtype == np.uint8
        assert got.shape == ((h, w) if channels == 1 else (h, w, channels))
        assert np.array_equal(got.reshape(h, w, channels), img), (ftype, channels, h, w)


def test_read_png_round_trips_write_png_and_multi_idat(tmp_path):
    from pano_nerf_amd import io_exr
    rng = np.random.default_rng(3)
    for shape in ((5, 3, 3), (4, 6), (2, 3, 4)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        path = str(tmp_path / "rt.png")
        io_exr.write_png(path, img)
        assert np.array_equal(io_exr.read_png(path), img)
    img = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    path = str(tmp_path / "multi.png")
    with open(path, "wb") as f:
        f.write(_png(img, None, idat_split=7))
    assert np.array_equal(io_exr.read_png(path), img)


def test_read_png_refusals(tmp_path):
    from pano_nerf_amd import io_exr
    img = np.zeros((2, 2, 3), np.uint8)
    cases = dict(sixteen=(_png(img, 0, depth=16), "16-bit"), palette=(_png(img[:, :, :1], 0, ctype=3), "palette"),
                 interlaced=(_png(img, 0, interlace=1), "interlaced"))
    for name, (blob, what) in cases.items():
        path = str(tmp_path / f"{name}.png")
        with open(path, "wb") as f:
            f.write(blob)
        with pytest.raises(NotImplementedError, match=what):
            io_exr.read_png(path)
    path = str(tmp_path / "not.png")
    with open(path, "wb") as f:
        f.write(b"P6 2 2 255\n" + bytes(12))
    with pytest.raises(ValueError, match="not a PNG"):
        io_exr.read_png(path)


# ------------------------------------------------------------------------------------------------------ read_obj
QUAD = """# a quad and a pentagon
mtllib mats.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0.5 1.5 0
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vt 0.5 1.5
vt 2 2
usemtl wood
f 1/1 2/2 3/3 4/4
usemtl paint
f 1/6 2/2 3/3 5/5 4/4
"""

MTL = """newmtl wood
Kd 0.5 0.25 0.125
Ns 10
map_Kd -s 1 1 1 -clamp on tex/wood.png
Pr 0.4
map_Pr rough.png
map_Bump -bm 0.5 bump.png

newmtl paint
Kd 1 0 0
norm n.png
illum 2
"""


def test_read_obj_polygons_materials_and_separate_vt(tmp_path):
    from pano_nerf_amd import geometry
    (tmp_path / "m.obj").write_text(QUAD)
    (tmp_path / "mats.mtl").write_text(MTL)
    m = geometry.read_obj(str(tmp_path / "m.obj"))
    assert m.vertices.shape == (5, 3) and m.vertices.dtype == np.float32
    assert m.faces.dtype == np.int32 and m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 4], [0, 4, 3]]
    assert m.face_uv.dtype == np.int32 and m.face_uv.tolist() == [[0, 1, 2], [0, 2, 3], [5, 1, 2], [5, 2, 4], [5, 4, 3]]
    assert m.uv.shape == (6, 2) and m.uv[5].tolist() == [2.0, 2.0]
    assert m.face_material.tolist() == [0, 0, 1, 1, 1]
    assert list(m.materials) == ["wood", "paint"]
    wood, paint = m.materials["wood"], m.materials["paint"]
    assert wood["Kd"] == (0.5, 0.25, 0.125) and wood["Pr"] == 0.4
    assert wood["map_Kd"] == os.path.join(str(tmp_path), "tex/wood.png")
    assert wood["map_Pr"] == os.path.join(str(tmp_path), "rough.png")
    assert wood["norm"] == os.path.join(str(tmp_path), "bump.png")
    assert paint["Kd"] == (1.0, 0.0, 0.0) and paint["Pr"] is None and paint["map_Kd"] is None
    assert paint["norm"] == os.path.join(str(tmp_path), "n.png")
    # no vn: area-weighted normals; the mesh is flat, so +z everywhere
    assert np.allclose(m.normals, [[0, 0, 1]] * 5, atol=1e-6)


def test_read_obj_corner_forms_negative_indices_and_normals(tmp_path):
    from pano_nerf_amd import geometry
    # v//vn with vn indices equal to the v indices: the file's normals are kept as they are
    (tmp_path / "a.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 -1\nvn 0 1 0\nvn 1 0 0\nf 1//1 2//2 3//3\n")
    a = geometry.read_obj(str(tmp_path / "a.obj"))
    assert a.faces.tolist() == [[0, 1, 2]] and a.uv is None and a.face_uv is None
    assert a.normals.tolist() == [[0, 0, -1], [0, 1, 0], [1, 0, 0]]
    assert a.face_material.tolist() == [-1] and len(a.materials) == 0
    # v/vt/vn with other vn indices: area-weighted normals instead; plain v; negative indices
    (tmp_path / "b.obj").write_text(
        "v 0 0 0\nv 2 0 0\nv 0 2 0\nvt 0 0\nvt 1 0\nvt 0 1\nvn 0 0 -1\nf -3/-3/-1 -2/-2/-1 -1/-1/-1\n"
        "v 0 0 1\nf 1/1/1 2/2/1 -1/3/1\n")
    b = geometry.read_obj(str(tmp_path / "b.obj"))
    assert b.faces.tolist() == [[0, 1, 2], [0, 1, 3]] and b.face_uv.tolist() == [[0, 1, 2], [0, 1, 2]]
    n0 = np.array([0, 0, 4.0]) + np.array([0, -2.0, 0])  # e1 x e2 of the two faces at vertex 0
    assert np.allclose(b.normals[0], n0 / np.linalg.norm(n0), atol=1e-6)
    assert np.allclose(b.normals[2], [0, 0, 1], atol=1e-6) and np.allclose(b.normals[3], [0, -1, 0], atol=1e-6)
    (tmp_path / "c.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\nf 1 -1 -2\n")
    c = geometry.read_obj(str(tmp_path / "c.obj"))
    assert c.faces.tolist() == [[0, 1, 2], [0, 2, 1]] and c.uv is None
    # one corner without vt: no UVs at all
    (tmp_path / "d.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2 3\n")
    assert geometry.read_obj(str(tmp_path / "d.obj")).uv is None


def test_read_obj_errors(tmp_path):
    from pano_nerf_amd import geometry
    (tmp_path / "lib.obj").write_text("mtllib nowhere.mtl\nv 0 0 0\n")
    with pytest.raises(FileNotFoundError, match="nowhere.mtl"):
        geometry.read_obj(str(tmp_path / "lib.obj"))
    (tmp_path / "idx.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError, match="index 4"):
        geometry.read_obj(str(tmp_path / "idx.obj"))
    (tmp_path / "zero.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n")
    with pytest.raises(ValueError, match="index 0"):
        geometry.read_obj(str(tmp_path / "zero.obj"))
    (tmp_path / "bad.obj").write_text("v 0 0 x\n")
    with pytest.raises(ValueError, match="unreadable line"):
        geometry.read_obj(str(tmp_path / "bad.obj"))
    # a usemtl name no library defines still gets an (empty) entry
    (tmp_path / "use.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl ghost\nf 1 2 3\n")
    m = geometry.read_obj(str(tmp_path / "use.obj"))
    assert list(m.materials) == ["ghost"] and m.materials["ghost"]["Kd"] is None and m.face_material.tolist() == [0]


# --------------------------------------------------------------------------------------------- the reference itself
def test_reference_tables_and_pyramid():
    lin, srgb = ref.decode_table(False), ref.decode_table(True)
    assert lin.dtype == np.float32 and lin[0] == 0 and lin[255] == 1 and lin[51] == np.float32(0.2)
    assert srgb[0] == 0 and srgb[255] == 1 and abs(float(srgb[128]) - 0.2158605) < 1e-6 and srgb[10] == np.float32(10 / 255 / 12.92)
    assert [ref.num_levels(*s) for s in ((1, 1), (2, 2), (5, 3), (3, 8), (64, 64), (16384, 1))] == [1, 2, 3, 4, 7, 15]
    assert ref.level_shapes(5, 3) == [(0, 5, 3), (15, 2, 1), (17, 1, 1)]
    img = np.arange(15, dtype=np.float32).reshape(5, 3)
    lv = ref.pyramid(ref.level0(img))
    assert [l.shape for l in lv] == [(5, 3, 4), (2, 1, 4), (1, 1, 4)]
    assert lv[0][2, 1].tolist() == [7.0, 0.0, 0.0, 1.0]
    assert lv[1][:, 0, 0].tolist() == [(0 + 1 + 3 + 4) / 4, (6 + 7 + 9 + 10) / 4]  # rows 0-1 and 2-3, columns 0-1
    assert lv[2][0, 0, 0] == (2.0 + 2.0 + 8.0 + 8.0) / 4 and lv[2][0, 0, 3] == 1.0  # the one column is read twice
    rgba = ref.level0(np.array([[[255, 0, 51, 51]]], np.uint8), srgb=True)
    assert rgba[0, 0].tolist() == [1.0, 0.0, float(srgb[51]), float(np.float32(0.2))]  # alpha is never gamma-decoded


def test_reference_bilinear_on_a_2x2_texture():
    lvl = np.zeros((2, 2, 4))
    lvl[..., 0] = [[1.0, 2.0], [3.0, 4.0]]
    for (U, V), want in (((0.25, 0.25), 1.0), ((0.75, 0.25), 2.0), ((0.25, 0.75), 3.0), ((0.75, 0.75), 4.0)):
        for wrap in ("repeat", "clamp"):
            assert ref.bilinear(lvl, U, V, wrap)[0] == want  # texel centres
    assert ref.bilinear(lvl, 0.5, 0.5, "repeat")[0] == 2.5
    # the seam U = 0: repeat blends the last and the first column half and half, clamp stays on the first
    assert ref.bilinear(lvl, 0.0, 0.25, "repeat")[0] == 1.5 and ref.bilinear(lvl, 0.0, 0.25, "clamp")[0] == 1.0
    assert ref.bilinear(lvl, 1.0, 0.75, "repeat")[0] == 3.5 and ref.bilinear(lvl, 1.0, 0.75, "clamp")[0] == 4.0
    # a whole period away is the same sample
    assert ref.bilinear(lvl, -0.75, 2.25, "repeat")[0] == ref.bilinear(lvl, 0.25, 0.25, "repeat")[0]
    levels = [lvl, np.full((1, 1, 4), 2.5)]
    assert ref.trilinear(levels, 0.5, 0.25, 0.25, "repeat")[0] == 0.5 * 1.0 + 0.5 * 2.5
    assert ref.trilinear(levels, 1.0, 0.25, 0.25, "repeat")[0] == 2.5


def test_reference_lod_of_a_unit_quad():
    """A unit square mapped to the whole of a 16 x 16 texture, seen head on: one texel is 1 / 16 wide, so a footprint of
    1 / 16 is level 0, of 1 / 4 level 2; tilting to cos = 1 / 2 adds a level."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    uv = v[:, :2].copy()
    tex = ref.pyramid(ref.level0(np.random.default_rng(0).random((16, 16, 3)).astype(np.float32)))
    down = np.array([0.0, 0.0, -2.0])
    tilt = np.array([0.0, math.sqrt(3.0), -1.0])
    rows = [(down, 1.0 / 32, 1.0, 0.0), (down, 1.0 / 16, 2.0, 2.0), (tilt, 1.0 / 16, 2.0, 3.0), (down, 1e-9, 1.0, 0.0),
            (down, 100.0, 1.0, 4.0)]
    R = len(rows)
    out = ref.texture_hits(np.ones(R, bool), np.zeros(R, np.int32), np.full((R, 2), 0.25), [r[0] for r in rows],
                           [r[2] for r in rows], np.tile([0.0, 0.0, 1.0], (R, 1)), [r[1] for r in rows], v, f, uv, None,
                           dict(albedo=tex), "repeat", False)
    assert np.allclose(out["lod"][:, 0], [r[3] for r in rows], atol=1e-12), out["lod"][:, 0]
    assert np.all(out["lod"][:, 1:] == 0)
    # no radii: level 0; level 4 is the mean texel
    none = ref.texture_hits(np.ones(1, bool), np.zeros(1, np.int32), np.full((1, 2), 0.25), [down], [1.0],
                            [[0.0, 0.0, 1.0]], None, v, f, uv, None, dict(albedo=tex), "repeat", False)
    assert none["lod"][0, 0] == 0.0
    assert np.allclose(out["albedo"][4], tex[4][0, 0, :3], atol=1e-7)
    # a flat normal map keeps N; a degenerate UV triangle keeps N and reads level 0
    flat = ref.pyramid(ref.level0(np.tile(np.array([0.5, 0.5, 1.0], np.float32), (4, 4, 1))))
    nm = ref.texture_hits(np.ones(2, bool), np.array([0, 1], np.int32), np.full((2, 2), 0.25), [down, down], [1.0, 1.0],
                          np.tile([0.0, 0.0, 1.0], (2, 1)), [0.01, 0.01], v, f, np.array([[0, 0], [1, 0], [1, 1], [2, 2]]),
                          None, dict(normal=flat), "repeat", False)
    assert np.allclose(nm["normals"], [[0, 0, 1], [0, 0, 1]], atol=1e-15)
    assert nm["fallback"].tolist() == [False, True] and nm["lod"][1, 2] == 0.0
