"""The OpenEXR reader on what datasets contain: FLOAT / HALF, NO_COMPRESSION / ZIPS / ZIP, any channel set, either
lineOrder, a dataWindow away from 0 - checked against files this test assembles itself, byte by byte, from the format
description (its encoder shares no code with the package), and the writer's new arguments by round trips."""
import struct
import zlib

import numpy as np
import pytest

from pano_nerf_amd import io_exr

MAGIC = 20000630


def attr(name, typ, payload):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(payload)) + payload


def zip_block(raw):
    """Straight-line OpenEXR ZIP: even bytes then odd bytes, each byte minus its predecessor plus 128, deflate."""
    n = len(raw)
    t = bytearray(n)
    a, b = 0, (n + 1) // 2
    for i in range(n):
        if i % 2 == 0:
            t[a] = raw[i]
            a += 1
        else:
            t[b] = raw[i]
            b += 1
    d = bytearray(n)
    d[0] = t[0]
    for i in range(1, n):
        d[i] = (t[i] - t[i - 1] + 128) % 256
    out = zlib.compress(bytes(d), 9)
    return out if len(out) < n else raw


def build_exr(chans, compression=0, x0=0, y0=0, decreasing=False, version=2):
    """chans: {name: [H, W] float16 / float32 array} -> bytes of a scanline file (channels stored alphabetically)."""
    names = sorted(chans)
    h, w = chans[names[0]].shape
    chlist = b""
    for n in names:
        ptype = {np.dtype(np.float16): 1, np.dtype(np.float32): 2, np.dtype(np.uint32): 0}[chans[n].dtype]
        chlist += n.encode() + b"\0" + struct.pack("<iBBBBii", ptype, 0, 0, 0, 0, 1, 1)
    chlist += b"\0"
    box = struct.pack("<iiii", x0, y0, x0 + w - 1, y0 + h - 1)
    head = struct.pack("<ii", MAGIC, version)
    head += attr("channels", "chlist", chlist) + attr("compression", "compression", bytes([compression]))
    head += attr("dataWindow", "box2i", box) + attr("displayWindow", "box2i", box)
    head += attr("lineOrder", "lineOrder", bytes([1 if decreasing else 0]))
    head += attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    head += attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0))
    head += attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"
    lines = 16 if compression == 3 else 1
    blocks = []
    for top in range(0, h, lines):
        raw = b"".join(chans[n][y].tobytes() for y in range(top, min(top + lines, h)) for n in names)
        blocks.append((y0 + top, zip_block(raw) if compression in (2, 3) else raw))
    order = list(reversed(blocks)) if decreasing else blocks  # the chunks lie in the file in lineOrder
    at = len(head) + 8 * len(blocks)
    where = {}
    body = b""
    for y, blob in order:
        where[y] = at + len(body)
        body += struct.pack("<ii", y, len(blob)) + blob
    table = b"".join(struct.pack("<Q", where[y]) for y, _ in blocks)  # the offset table is by increasing y
    return head + table + body


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("compression", ["none", "zips", "zip"])
@pytest.mark.parametrize("shape", [(5, 7), (37, 30), (16, 32)])
def test_write_read_round_trip(tmp_path, compression, half, shape):
    rng = np.random.default_rng(hash((compression, half, shape)) % 2**32)
    d = (rng.standard_normal(shape + (3,)) * 10).astype(np.float32)
    name = str(tmp_path / "a.exr")
    io_exr.write_exr(name, d, compression=compression, half=half)
    want = d.astype(np.float16).astype(np.float32) if half else d
    assert np.array_equal(io_exr.read_exr(name), want)
    planes, names, types = io_exr.read_exr_planes(name)
    assert names == ["B", "G", "R"] and types == ["half" if half else "float"] * 3
    assert planes.dtype == (np.float16 if half else np.float32) and planes.shape == (shape[0], 3, shape[1])
    assert np.array_equal(planes[:, 2, :].astype(np.float32), want[:, :, 0])


def test_compressed_files_are_smaller(tmp_path):
    d = np.tile(np.linspace(0, 1, 64, dtype=np.float32)[None, :, None], (32, 1, 3))
    sizes = {}
    for c in ("none", "zips", "zip"):
        io_exr.write_exr(str(tmp_path / f"{c}.exr"), d, compression=c)
        sizes[c] = (tmp_path / f"{c}.exr").stat().st_size
    assert sizes["zip"] < sizes["zips"] < sizes["none"]


@pytest.mark.parametrize("compression", [0, 2, 3])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_independent_encoder_is_read_exactly(tmp_path, compression, dtype):
    rng = np.random.default_rng(compression * 2 + (dtype is np.float16))
    h, w = 21, 13
    # smooth planes deflate, a noise plane does not: both the compressed and the stored-raw block paths are read
    chans = {"R": np.linspace(0, 4, h * w).reshape(h, w).astype(dtype), "G": rng.standard_normal((h, w)).astype(dtype),
             "B": np.full((h, w), 0.25, dtype), "A": rng.uniform(0, 1, (h, w)).astype(dtype),
             "Z": np.zeros((h, w), dtype)}
    name = str(tmp_path / "b.exr")
    open(name, "wb").write(build_exr(chans, compression))
    got = io_exr.read_exr(name)
    for k, c in enumerate("RGB"):
        assert np.array_equal(got[:, :, k], chans[c].astype(np.float32))
    assert np.array_equal(io_exr.read_exr(name, channel=1)[:, :, 0], chans["A"].astype(np.float32))
    planes, names, _ = io_exr.read_exr_planes(name)
    assert names == ["A", "B", "G", "R", "Z"] and planes.dtype == dtype
    assert np.array_equal(planes[:, 3, :], chans["R"])


def test_noise_block_is_stored_raw(tmp_path):
    raw = np.random.default_rng(3).integers(0, 256, 4 * 13 * 3, dtype=np.uint8).tobytes()
    assert zip_block(raw) == raw  # (the precondition of the stored-raw path above)


def test_mixed_pixel_types(tmp_path):
    h, w = 4, 6
    rng = np.random.default_rng(9)
    chans = {"R": rng.standard_normal((h, w)).astype(np.float16), "G": rng.standard_normal((h, w)).astype(np.float32),
             "B": rng.standard_normal((h, w)).astype(np.float16)}
    name = str(tmp_path / "m.exr")
    open(name, "wb").write(build_exr(chans, 3))
    got = io_exr.read_exr(name)
    for k, c in enumerate("RGB"):
        assert np.array_equal(got[:, :, k], chans[c].astype(np.float32))
    planes, names, types = io_exr.read_exr_planes(name)
    assert planes.dtype == np.float32 and types == ["float"] * 3


@pytest.mark.parametrize("compression", [0, 3])
def test_data_window_offset_and_decreasing_y(tmp_path, compression):
    rng = np.random.default_rng(11)
    h, w = 35, 10
    chans = {c: rng.standard_normal((h, w)).astype(np.float32) for c in "RGB"}
    name = str(tmp_path / "c.exr")
    open(name, "wb").write(build_exr(chans, compression, x0=-7, y0=19, decreasing=True))
    got = io_exr.read_exr(name)
    assert got.shape == (h, w, 3)
    for k, c in enumerate("RGB"):
        assert np.array_equal(got[:, :, k], chans[c])


def test_piz_is_named(tmp_path):
    chans = {c: np.zeros((2, 2), np.float32) for c in "RGB"}
    name = str(tmp_path / "p.exr")
    open(name, "wb").write(build_exr(chans, 4))
    with pytest.raises(NotImplementedError, match="PIZ"):
        io_exr.read_exr(name)
    open(name, "wb").write(build_exr(chans, 1))
    with pytest.raises(NotImplementedError, match="RLE"):
        io_exr.read_exr_planes(name)


@pytest.mark.parametrize("bit,what", [(0x200, "tiled"), (0x800, "deep"), (0x1000, "multi-part")])
def test_other_file_kinds_raise(tmp_path, bit, what):
    chans = {c: np.zeros((2, 2), np.float32) for c in "RGB"}
    name = str(tmp_path / "t.exr")
    open(name, "wb").write(build_exr(chans, 0, version=2 | bit))
    with pytest.raises(NotImplementedError, match=what):
        io_exr.read_exr(name)


def test_uint_channels_raise(tmp_path):
    chans = {"R": np.zeros((2, 2), np.uint32), "G": np.zeros((2, 2), np.float32), "B": np.zeros((2, 2), np.float32)}
    name = str(tmp_path / "u.exr")
    open(name, "wb").write(build_exr(chans, 0))
    with pytest.raises(NotImplementedError, match="UINT"):
        io_exr.read_exr(name)


def test_default_writer_bytes_are_unchanged(tmp_path):
    """write_exr(name, data) = the documented layout: B, G, R FLOAT channels, NO_COMPRESSION, increasing Y, one block per
    line - the bytes it wrote before it learned compression and HALF."""
    rng = np.random.default_rng(5)
    d = rng.standard_normal((6, 9, 3)).astype(np.float32)
    name = str(tmp_path / "d.exr")
    io_exr.write_exr(name, d)
    want = build_exr({"R": d[:, :, 0].copy(), "G": d[:, :, 1].copy(), "B": d[:, :, 2].copy()}, 0)
    assert open(name, "rb").read() == want
    with pytest.raises(TypeError):
        io_exr.write_exr(name, d, "zip")  # the new arguments are keyword-only
    with pytest.raises(ValueError):
        io_exr.write_exr(name, d, compression="piz")
