"""The per-triangle texture atlas without a GPU: the numpy restatement of the layout (tests/_atlas_ref.py) against the
properties the layout was designed for, and the host code of pano_nerf_amd.geometry (cell choice, write_obj / read_obj).

The tap property is checked with the sampler's own bilinear rule (tests/_textures_ref.bilinear) on an image that is 1 on
every texel the face does NOT own: the sample is exactly 0 iff every tap with a non-zero weight is the face's own.  It is
exact where the arithmetic is - atlas sizes that are powers of two, sample points given in texel coordinates with a few
binary digits - and holds up to the weight a rounded coordinate can give a fifth tap (<= 1e-9) for other sizes."""
import os

import numpy as np
import pytest

import _atlas_ref as ref
import _textures_ref as tref


# ---------------------------------------------------------------------------------------------------- cell choice
@pytest.mark.parametrize("S", [6, 16, 37, 64, 100, 1024])
def test_cell_choice(S):
    from pano_nerf_amd import geometry
    top = ref.capacity(S, ref.MIN_CELL)
    for F in sorted({1, 2, 3, 7, 8, 9, 130, top - 1, top}):
        if F < 1 or F > top:
            continue
        c = geometry.atlas_cell(F, S)
        assert c == ref.cell_size(F, S), (S, F)
        assert c >= ref.MIN_CELL and ref.capacity(S, c) >= F and (c == S or ref.capacity(S, c + 1) < F)
    with pytest.raises(ValueError) as e:
        geometry.atlas_cell(top + 1, S)  # one above the capacity at the smallest cell
    need = ref.smallest_size(top + 1)
    assert need > S and str(need) in str(e.value), (str(e.value), need)
    assert geometry.atlas_cell(top + 1, need) == ref.MIN_CELL


def test_cell_choice_rejects_bad_sizes():
    from pano_nerf_amd import geometry
    for S in (0, -3, 5, 16385):
        with pytest.raises(ValueError):
            geometry.atlas_cell(1, S)
    assert geometry.ATLAS_MIN_CELL == ref.MIN_CELL and geometry.ATLAS_MAX_SIZE == ref.MAX_SIZE


# ------------------------------------------------------------------------------------------ triangles in their cells
@pytest.mark.parametrize("S,F", [(6, 2), (16, 8), (37, 7), (37, 72), (64, 130), (100, 512)])
def test_uv_triangles_lie_inside_their_cells(S, F):
    c = ref.cell_size(F, S)
    n = S // c
    xy = ref.atlas_xy(F, S, c)
    uv = ref.atlas_uv(F, S, c).reshape(F, 3, 2)
    for f in range(F):
        k = f // 2
        org = np.array([(k % n) * c, (k // n) * c], np.float64)
        loc = xy[f] - org
        assert np.all(loc >= ref.MARGIN) and np.all(loc <= c - ref.MARGIN), (f, loc)
        s = loc.sum(1)
        # DIAG texels between the hypotenuses: triangle 0 below x + y = c - 2 + ..., triangle 1 above
        assert (np.all(s <= c - ref.DIAG) if f % 2 == 0 else np.all(s >= c + ref.DIAG)), (f, s)
        assert org[0] + c <= n * c <= S and org[1] + c <= n * c
        # legs of L texels along x (corner 1) and y (corner 2); the UVs restate the same corners in OBJ's convention
        L = c - 2 * ref.MARGIN - ref.DIAG
        sign = 1 if f % 2 == 0 else -1
        np.testing.assert_array_equal(loc[1] - loc[0], (sign * L, 0))
        np.testing.assert_array_equal(loc[2] - loc[0], (0, sign * L))
        np.testing.assert_allclose(uv[f, :, 0] * S, xy[f, :, 0], rtol=0, atol=1e-9)
        np.testing.assert_allclose((1 - uv[f, :, 1]) * S, xy[f, :, 1], rtol=0, atol=1e-9)


def test_ownership_partitions_the_cells():
    for S, F in ((16, 8), (37, 7), (64, 130)):
        c = ref.cell_size(F, S)
        n = S // c
        face, u, v = ref.owners(S, c, F)
        assert np.all(face[n * c:] == -1) and np.all(face[:, n * c:] == -1)
        counts = np.bincount(face[face >= 0], minlength=F)
        # a cell's c^2 texels: the c (c - 1) / 2 with li + lj + 1 < c go to triangle 0, the rest to triangle 1
        assert np.all(counts[0::2] == c * (c - 1) // 2) and np.all(counts[1::2] == c * (c + 1) // 2)
        # texels inside a triangle (all three barycentrics >= 0) exist for every face
        inside = (face >= 0) & (u >= 0) & (v >= 0) & (1 - u - v >= 0)
        assert np.all(np.bincount(face[inside], minlength=F) >= 1)


# ------------------------------------------------------------------------------------------------ the tap property
def sample_points(h, c, rng, count=24):
    """points (x, y) of the closed triangle h of a cell, in cell texel coordinates, each a multiple of 2^-10"""
    P = ref.corners(h, c)
    L = c - 2 * ref.MARGIN - ref.DIAG
    pts = [P[0], P[1], P[2], (P[0] + P[1]) / 2, (P[0] + P[2]) / 2, (P[1] + P[2]) / 2]
    for k in range(2 * L + 1):  # the hypotenuse from P1 to P2 in half-texel steps
        t = 0.5 * k
        pts.append(P[1] + (np.array([-t, t]) if h == 0 else np.array([t, -t])))
    for k in range(2 * L + 1):  # and both legs
        t = 0.5 * k * (1 if h == 0 else -1)
        pts += [P[0] + np.array([t, 0.0]), P[0] + np.array([0.0, t])]
    a, b = rng.random(count), rng.random(count)
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    q = np.round(np.stack([a, b], 1) * L * 1024) / 1024  # bary (u, v) L on the 2^-10 grid, still u + v <= 1 (rounding
    q = q[q.sum(1) <= L]                                  # to a grid that holds L keeps the bound; drop the rest anyway)
    sign = 1.0 if h == 0 else -1.0
    pts += [P[0] + sign * r for r in q]
    return np.asarray(pts, np.float64)


def foreign_tap_weight(S, c, F, rng):
    """max over faces and sample points of the bilinear sample of (1 on texels the face does not own)"""
    n = S // c
    face, _, _ = ref.owners(S, c, F)
    worst = 0.0
    for f in range(F):
        img = np.zeros((S, S, 4), np.float32)
        img[..., 0] = face != f
        org = ref.cell_origin(f, S, c)
        for p in sample_points(f & 1, c, rng):
            X, Y = org + p
            U, V = X / S, 1.0 - Y / S  # the UV of the point; the sampler flips V back (flip_v)
            worst = max(worst, float(tref.bilinear(img, U, 1.0 - V, "repeat")[0]))
    return worst


@pytest.mark.parametrize("c,S", [(6, 16), (7, 16), (8, 16), (13, 32)])
def test_tap_property_exact(c, S):
    """power-of-two sizes: X / S and 1 - Y / S are exact, so is U S - 0.5: not one foreign tap, whatever its weight"""
    n = S // c
    assert n == 2
    rng = np.random.default_rng(c)
    for F in (1, 2, 3, 2 * n * n):
        assert foreign_tap_weight(S, c, F, rng) == 0.0, (c, F)


@pytest.mark.parametrize("c,S,F", [(6, 6, 2), (6, 64, 200), (7, 37, 50), (13, 100, 98), (9, 64, 98)])
def test_tap_property_other_sizes(c, S, F):
    """any size: a rounded U S can leave the texel grid by ~1e-14 texels and hand a further tap that weight at most"""
    assert ref.capacity(S, c) >= F
    assert foreign_tap_weight(S, c, F, np.random.default_rng(S)) <= 1e-9


def test_tap_property_fails_without_the_margins():
    """the check has teeth: a layout whose corners sit on the cell's border reads the neighbours"""
    S, c, F = 16, 8, 8
    face, _, _ = ref.owners(S, c, F)
    img = np.zeros((S, S, 4), np.float32)
    img[..., 0] = face != 0
    assert float(tref.bilinear(img, 0.0 / S, 0.0 / S, "repeat")[0]) > 0.5       # the cell's corner: wraps around
    assert float(tref.bilinear(img, 4.0 / S, 4.0 / S, "repeat")[0]) > 0.2       # on the cell's diagonal x + y = c


# --------------------------------------------------------------------------------------------------- the quantiser
@pytest.mark.parametrize("srgb", [False, True])
def test_quantiser_finds_the_nearest_code(srgb):
    t = tref.decode_table(srgb)
    assert np.all(np.diff(t.astype(np.float64)) > 0) and t[0] == 0.0 and t[255] == 1.0
    mid = ((t[:-1].astype(np.float64) + t[1:].astype(np.float64)) / 2).astype(np.float32)
    x = np.concatenate([t, mid])
    x = np.concatenate([x, np.nextafter(x, np.float32(-1)), np.nextafter(x, np.float32(2)),
                        np.array([-1.0, -0.0, 1.5, np.inf, -np.inf, np.nan, 1e-30, 0.999999], np.float32),
                        np.random.default_rng(0).random(4096).astype(np.float32)]).astype(np.float32)
    got, want = ref.quantize(x, t), ref.quantize_brute(x, t)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(ref.quantize(t, t), np.arange(256))  # decode then encode is the identity
    # exact ties go to the lower code: midpoints that are representable (the linear table's are not all; check those that are)
    exact = (mid.astype(np.float64) - t[:-1]) == (t[1:].astype(np.float64) - mid)
    np.testing.assert_array_equal(ref.quantize(mid[exact], t), np.arange(255)[exact])
    bad = np.array([np.nan, -3.0, -np.inf], np.float32)
    assert np.all(ref.quantize(bad, t) == 0) and np.all(ref.quantize(np.array([7.0, np.inf], np.float32), t) == 255)


def test_quantiser_without_a_table_rounds_half_to_even():
    k = np.arange(255, dtype=np.float64)
    x = np.concatenate([((k + 0.5) / 255.0).astype(np.float32), (k / 255.0).astype(np.float32),
                        np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, np.nan, -1.0, 2.0], np.float32),
                        np.random.default_rng(1).random(2048).astype(np.float32)])
    want = []
    for v in x:
        v = 0.0 if not v > 0 else min(float(v), 1.0)
        want.append(round(255.0 * v))  # python's round: half to even, on the exact product (255 x has <= 32 bits)
    np.testing.assert_array_equal(ref.quantize(x), np.asarray(want, np.uint8))
    # exact halves exist: 0.5 = 127.5 / 255 -> 128 (even), and x = 2^-k multiples that hit k + 0.5 exactly
    assert ref.quantize(np.array([0.5], np.float32))[0] == 128


# ------------------------------------------------------------------------------------------- write_obj -> read_obj
def host_baked(with_normals, fmt):
    from pano_nerf_amd import geometry
    rng = np.random.default_rng(5)
    v = (rng.normal(size=(6, 3)) * np.array([1.0, 1e-3, 1e3])).astype(np.float32)
    v[0] = (0.1, 1.0 / 3.0, -2.0 / 3.0)  # not representable in a few decimal digits
    f = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 5], [5, 0, 2], [1, 4, 3]], np.int32)
    n = rng.normal(size=(6, 3)).astype(np.float32) if with_normals else None
    S = 16
    c = geometry.atlas_cell(len(f), S)
    uv = ref.f32(ref.atlas_uv(len(f), S, c))
    fuv = np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)
    if fmt == "png":
        maps = dict(albedo=rng.integers(0, 256, (S, S, 3), dtype=np.uint8), normal=rng.integers(0, 256, (S, S, 3), dtype=np.uint8))
    else:
        maps = dict(albedo=rng.random((S, S, 3)).astype(np.float32), normal=rng.random((S, S, 3)).astype(np.float32))
    maps["radiance"] = (rng.random((S, S, 3)) * 30).astype(np.float32)
    maps["coverage"] = np.ones((S, S, 1), np.float32)
    return geometry.BakedMesh(v, f, n, uv, fuv, maps)


@pytest.mark.parametrize("fmt", ["png", "exr"])
@pytest.mark.parametrize("with_normals", [True, False])
def test_write_obj_read_obj_round_trip(tmp_path, with_normals, fmt):
    from pano_nerf_amd import geometry, io_exr
    b = host_baked(with_normals, fmt)
    path = str(tmp_path / "scene.obj")
    files = geometry.write_obj(path, b, image_format=fmt)
    m = geometry.read_obj(path)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    np.testing.assert_array_equal(bits(m.vertices), bits(b.vertices))
    np.testing.assert_array_equal(m.faces, b.faces)
    np.testing.assert_array_equal(bits(m.uv), bits(b.uv))
    np.testing.assert_array_equal(m.face_uv, b.face_uv)
    if with_normals:
        np.testing.assert_array_equal(bits(m.normals), bits(b.normals))
    assert list(m.materials) == ["scene"] and np.all(m.face_material == 0)
    mat = m.materials["scene"]
    assert os.path.basename(mat["map_Kd"]) == f"scene_albedo.{fmt}" and os.path.basename(mat["norm"]) == f"scene_normal.{fmt}"
    assert mat["map_Pr"] is None
    assert sorted(files) == ["albedo", "normal", "radiance"] and files["radiance"].endswith("scene_radiance.exr")
    for k, p in files.items():
        assert os.path.isfile(p), p
    assert not os.path.exists(str(tmp_path / "scene_coverage.png"))
    if fmt == "png":
        np.testing.assert_array_equal(io_exr.read_png(mat["map_Kd"]), b.maps["albedo"])
        np.testing.assert_array_equal(io_exr.read_png(mat["norm"]), b.maps["normal"])
    else:
        np.testing.assert_array_equal(bits(io_exr.read_exr(mat["map_Kd"])), bits(b.maps["albedo"]))
        np.testing.assert_array_equal(bits(io_exr.read_exr(mat["norm"])), bits(b.maps["normal"]))
    np.testing.assert_array_equal(bits(io_exr.read_exr(files["radiance"])), bits(b.maps["radiance"]))


def test_write_obj_refuses_what_it_cannot_write(tmp_path):
    from pano_nerf_amd import geometry
    b = host_baked(False, "exr")
    with pytest.raises(RuntimeError, match="quantiser"):
        geometry.write_obj(str(tmp_path / "a.obj"), b, image_format="png")  # fp32 on the host: no CPU quantiser
    with pytest.raises(ValueError):
        geometry.write_obj(str(tmp_path / "a.obj"), b, image_format="jpg")
    with pytest.raises(ValueError):
        geometry.write_obj(str(tmp_path / "a.obj"), host_baked(False, "png"), image_format="exr")  # uint8 into EXR
