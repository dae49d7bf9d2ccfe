"""OpenEXR reader / writer and 8-bit PNG writer / reader for datasets, textures and validation dumps, with no third-party
codec.

`utils/io_exr.py:30-47` writes an RGB float32 scanline OpenEXR through the OpenEXR python binding and
`utils/io_exr.py:6-27` reads one back; the binding is not available here, so this module emits / parses the
container itself (OpenEXR 2 single-part scanline file, channels B G R as FLOAT, NO_COMPRESSION, increasing Y) —
the layout any OpenEXR reader accepts.  Parity with files written by the real library is unpinned (the library is
absent on both boxes): the tests check the header fields and a write -> read round trip.  SURVEY.md 8f rank 4.

The reader also takes what datasets contain (Blender writes ZIP-compressed, usually HALF files): FLOAT / HALF channels,
NO_COMPRESSION / ZIPS / ZIP, any channel set, either lineOrder, any dataWindow origin.  ZIP is zlib + a byte-delta
predictor + a two-halves byte interleave, all undone here.  The codec is checked against this writer and against an
independent encoder in the tests, NOT against files of the OpenEXR library: that parity stays unpinned too.
"""
import struct
import zlib

import numpy as np

_MAGIC = 20000630


def _attr(name, typ, payload):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(payload)) + payload


_COMPRESSION = {"none": 0, "zips": 2, "zip": 3}
_LINES = {0: 1, 2: 1, 3: 16}  # scanlines per block
_CODECS = {1: "RLE", 4: "PIZ", 5: "PXR24", 6: "B44", 7: "B44A", 8: "DWAA", 9: "DWAB"}
_PIXEL = {0: ("uint", np.uint32), 1: ("half", np.float16), 2: ("float", np.float32)}


def _zip_pack(raw):
    """OpenEXR's ZIP block: bytes split into (even, odd) halves, byte-delta predictor, deflate.  A block that does not
    shrink is stored raw."""
    a = np.frombuffer(raw, np.uint8)
    t = np.concatenate([a[0::2], a[1::2]])
    d = t.copy()
    d[1:] = t[1:] - t[:-1] + np.uint8(128)  # uint8 arithmetic wraps mod 256
    out = zlib.compress(d.tobytes(), 6)
    return out if len(out) < len(raw) else raw


def _zip_unpack(blob, raw_size):
    if len(blob) == raw_size:  # stored raw
        return blob
    d = np.frombuffer(zlib.decompress(blob), np.uint8).copy()
    if d.size != raw_size:
        raise ValueError(f"ZIP block inflates to {d.size} bytes, {raw_size} expected")
    d[1:] -= np.uint8(128)
    t = np.cumsum(d, dtype=np.uint8)  # t[i] = t[i-1] + d[i] - 128 mod 256
    half = (raw_size + 1) // 2
    out = np.empty(raw_size, np.uint8)
    out[0::2] = t[:half]
    out[1::2] = t[half:]
    return out.tobytes()


def write_exr(filename, data, *, compression="none", half=False):
    """data: float32 [H, W, 3] or [H, W, 1] (grey is replicated to R, G, B like upstream).  `compression` is "none",
    "zips" (one line per block) or "zip" (16 lines per block); `half=True` stores HALF channels (values are rounded).
    The defaults write the uncompressed FLOAT file this function has always written, byte for byte."""
    assert filename.endswith(".exr"), "extension must be .exr"
    data = np.asarray(data)
    assert data.dtype == np.float32, f"data type is {data.dtype}, should be float32"
    if compression not in _COMPRESSION:
        raise ValueError(f"compression must be one of {sorted(_COMPRESSION)}, got {compression!r}")
    comp = _COMPRESSION[compression]
    h, w, c = data.shape
    if c == 1:
        data = np.repeat(data, 3, axis=2)
    ptype, esize = (1, 2) if half else (2, 4)
    chlist = b"".join(n + b"\0" + struct.pack("<iBBBBii", ptype, 0, 0, 0, 0, 1, 1) for n in (b"B", b"G", b"R")) + b"\0"
    box = struct.pack("<iiii", 0, 0, w - 1, h - 1)
    header = (_attr("channels", "chlist", chlist) + _attr("compression", "compression", bytes([comp])) +
              _attr("dataWindow", "box2i", box) + _attr("displayWindow", "box2i", box) +
              _attr("lineOrder", "lineOrder", b"\0") + _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) +
              _attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0)) +
              _attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")
    head = struct.pack("<ii", _MAGIC, 2) + header
    bgr = np.ascontiguousarray(data[:, :, ::-1].transpose(0, 2, 1))  # [H][B,G,R][W]
    if half:
        bgr = bgr.astype(np.float16)
    lines = _LINES[comp]
    blocks = []
    for y in range(0, h, lines):
        raw = bgr[y:y + lines].tobytes()
        blocks.append((y, _zip_pack(raw) if comp else raw))
    first = len(head) + 8 * len(blocks)
    offsets, at = [], first
    for _, blob in blocks:
        offsets.append(at)
        at += 8 + len(blob)
    with open(filename, "wb") as f:
        f.write(head)
        f.write(struct.pack("<%dQ" % len(blocks), *offsets))
        for y, blob in blocks:
            f.write(struct.pack("<ii", y, len(blob)))
            f.write(blob)


def _decode(filename):
    """-> (list of [H, W] arrays, one per stored channel and in its stored type, names, pixel type names)."""
    with open(filename, "rb") as f:
        buf = f.read()
    magic, version = struct.unpack_from("<ii", buf, 0)
    if magic != _MAGIC or (version & 0xff) != 2:
        raise ValueError("not an OpenEXR 2 file")
    for bit, what in ((0x200, "tiled"), (0x800, "deep"), (0x1000, "multi-part")):
        if version & bit:
            raise NotImplementedError(f"{what} OpenEXR files are not read here (single-part scanline files only)")
    pos, attrs = 8, {}
    while buf[pos] != 0:
        end = buf.index(b"\0", pos)
        name = buf[pos:end].decode()
        pos = end + 1
        end = buf.index(b"\0", pos)
        pos = end + 1
        (size,) = struct.unpack_from("<i", buf, pos)
        attrs[name] = buf[pos + 4:pos + 4 + size]
        pos += 4 + size
    pos += 1
    comp = attrs["compression"][0]
    if comp not in _LINES:
        raise NotImplementedError(f"OpenEXR compression {_CODECS.get(comp, comp)} is not read here "
                                  "(NO_COMPRESSION, ZIPS and ZIP only)")
    names, types, p, ch = [], [], 0, attrs["channels"]
    while ch[p] != 0:
        end = ch.index(b"\0", p)
        ptype, _, xs, ys = struct.unpack_from("<i4sii", ch, end + 1)
        if ptype not in (1, 2):
            raise NotImplementedError(f"channel {ch[p:end].decode()!r} is {_PIXEL.get(ptype, (ptype,))[0].upper()}: "
                                      "only HALF and FLOAT channels are read here")
        if (xs, ys) != (1, 1):
            raise NotImplementedError("sub-sampled channels are not read here")
        names.append(ch[p:end].decode())
        types.append(ptype)
        p = end + 1 + 16
    x0, y0, x1, y1 = struct.unpack("<iiii", attrs["dataWindow"])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    lines = _LINES[comp]
    n_blocks = (h + lines - 1) // lines
    offsets = struct.unpack_from("<%dQ" % n_blocks, buf, pos)
    dts = [_PIXEL[t][1] for t in types]
    planes = [np.empty((h, w), dt) for dt in dts]
    line_bytes = sum(w * np.dtype(dt).itemsize for dt in dts)
    for off in offsets:  # a block carries its own first line, so either lineOrder reads the same way
        y, nbytes = struct.unpack_from("<ii", buf, off)
        rows = min(lines, y1 - y + 1)
        if not (y0 <= y <= y1) or (y - y0) % lines:
            raise ValueError(f"scanline block at y = {y} lies outside the dataWindow")
        blob = buf[off + 8:off + 8 + nbytes]
        raw = _zip_unpack(blob, rows * line_bytes) if comp else blob
        if len(raw) != rows * line_bytes:
            raise ValueError(f"scanline block at y = {y} holds {len(raw)} bytes, {rows * line_bytes} expected")
        at = 0
        for r in range(rows):
            for plane, dt in zip(planes, dts):
                plane[y - y0 + r] = np.frombuffer(raw, dt, w, at)
                at += w * np.dtype(dt).itemsize
    return planes, names, [_PIXEL[t][0] for t in types]


def read_exr_planes(filename):
    """The undecoded channel planes of a single-part scanline file -> (planes [H, n_ch, W], names, pixel_types).
    `planes` has the file's pixel type (float16 or float32; a file that mixes both is widened to float32, exactly),
    channels in stored (alphabetical) order: the layout `data.ingest_image` hands to the device."""
    planes, names, types = _decode(filename)
    if len(set(types)) > 1:
        planes, types = [p.astype(np.float32) for p in planes], ["float"] * len(types)
    return np.ascontiguousarray(np.stack(planes, axis=1)), names, types


def read_exr(filename, channel=3):
    """Single-part scanline OpenEXR (FLOAT or HALF channels; NO_COMPRESSION, ZIPS or ZIP; any channel set, lineOrder
    and dataWindow origin) -> float32 [H, W, channel]: R, G, B for channel == 3, A otherwise.  Tiled, multi-part and
    deep files, UINT channels and the codecs RLE, PIZ, PXR24, B44[A], DWAA/B raise NotImplementedError naming what was
    found.  Files written by the OpenEXR library itself are unpinned here for the same reason as the writer's."""
    planes, names, _ = _decode(filename)
    want = "RGB" if channel == 3 else "A"
    return np.stack([planes[names.index(c)].astype(np.float32) for c in want], axis=2)


def write_png(filename, img):
    """uint8 [H, W, 3] or [H, W] -> PNG (zlib only); float images in [0, 1] are scaled and TRUNCATED like
    `hdr_to_ldr(dtype='uint8')` (`utils/surface_rendering.py:319-344`)."""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        img = (np.clip(img, 0.0, 1.0) * 255).astype(np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, c = img.shape
    ctype = {1: 0, 3: 2, 4: 6}[c]
    raw = b"".join(b"\0" + img[y].tobytes() for y in range(h))

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xffffffff)

    with open(filename, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


_PNG_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}  # colour type -> samples per pixel
_PNG_COLOUR = {0: "greyscale", 2: "RGB", 3: "palette", 4: "grey + alpha", 6: "RGBA"}


def read_png(path):
    """8-bit, non-interlaced PNG (greyscale, grey + alpha, RGB or RGBA; all five filter types; any number of IDAT chunks)
    -> uint8 [H, W] for greyscale, [H, W, C] otherwise (C = 2, 3, 4), with zlib and numpy only.  16-bit (or 1 / 2 / 4-bit),
    palette and interlaced files raise NotImplementedError naming what was found; a file that is no PNG, or whose data ends
    early, raises ValueError.  Ancillary chunks (gAMA, sRGB, tEXt, ...) are skipped and CRCs are not checked."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos + 8 <= len(data):
        (n,), tag = struct.unpack_from(">I", data, pos), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
    if hdr is None:
        raise ValueError(f"{path}: no IHDR chunk")
    w, h, depth, ctype, _, _, interlace = hdr
    if ctype == 3:
        raise NotImplementedError(f"{path}: palette PNG files are not read here (8-bit greyscale, grey + alpha, RGB, RGBA only)")
    if ctype not in _PNG_CHANNELS:
        raise ValueError(f"{path}: unknown PNG colour type {ctype}")
    if depth != 8:
        raise NotImplementedError(f"{path}: {depth}-bit {_PNG_COLOUR[ctype]} PNG files are not read here (8-bit only)")
    if interlace:
        raise NotImplementedError(f"{path}: interlaced (Adam7) PNG files are not read here")
    c = _PNG_CHANNELS[ctype]
    stride = w * c
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    if raw.size < h * (stride + 1):
        raise ValueError(f"{path}: the image data holds {raw.size} bytes, {h * (stride + 1)} expected")
    rows = raw[:h * (stride + 1)].reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.uint8)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:]
        if ft == 0:
            cur = line.copy()
        elif ft == 1:  # Sub: each channel is a running sum along the row (uint8 arithmetic wraps mod 256)
            cur = np.cumsum(line.reshape(w, c), axis=0, dtype=np.uint8).reshape(stride)
        elif ft == 2:  # Up
            cur = line + prev
        elif ft in (3, 4):  # Average, Paeth: the left neighbour is the value just decoded
            cur = np.empty(stride, np.uint8)
            x_, up = line.astype(np.int32), prev.astype(np.int32)
            dec = [0] * stride
            for i in range(stride):
                a = dec[i - c] if i >= c else 0
                b = int(up[i])
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    cc = int(up[i - c]) if i >= c else 0
                    p = a + b - cc
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)
                dec[i] = (int(x_[i]) + pred) & 255
            cur[:] = dec
        else:
            raise ValueError(f"{path}: unknown filter type {ft} on row {y}")
        out[y] = cur
        prev = cur
    return out.reshape(h, w) if c == 1 else out.reshape(h, w, c)
