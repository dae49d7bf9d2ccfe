"""Audit of the numpy reference tests/_fill_ref.py (the header's hole-filling and blending rules) and of the scenes the GPU
tests use: the properties the rule is meant to have, on hand-checked cases.  No GPU."""
import numpy as np
import pytest

import _fill_ref as fr

F = np.float32
SIZES = fr.SIZES
DENSITIES = [0.02, 0.5, 0.98]
scene, background_scene = fr.scene, fr.background_scene


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("with_depth", [False, True])
def test_complete_and_within_range(size, density, wrap, with_depth):
    H, W = size
    img, dep, known = scene(H, W, density)
    out, od, filled = fr.fill_holes(img, dep if with_depth else None, known, None, wrap, 0.05, None)
    for n in range(img.shape[0]):
        k = known[n]
        if not k.any():
            assert not filled[n].any() and np.array_equal(bits(out[n]), bits(img[n]))
            continue
        assert np.array_equal(filled[n], ~k)  # fully known afterwards
        assert np.isfinite(out[n]).all()
        for c in range(img.shape[1]):
            lo, hi = img[n, c][k].min(), img[n, c][k].max()
            assert out[n, c].min() >= lo - 1e-6 and out[n, c].max() <= hi + 1e-6
            assert np.array_equal(bits(out[n, c][k]), bits(img[n, c][k]))
        if with_depth:
            assert np.isfinite(od[n]).all() and (od[n] > 0).all()
            assert od[n].min() >= dep[n][k].min() - 1e-6 and od[n].max() <= dep[n][k].max() + 1e-6
            assert np.array_equal(bits(od[n][k]), bits(dep[n][k]))
    assert od is None or with_depth


def test_background_is_preferred():
    img, dep, known = background_scene()
    hole = ~known[0]
    assert hole.sum() == 24
    out, od, filled = fr.fill_holes(img, dep, known)
    assert np.array_equal(filled[0], hole)
    assert (out[0, 0][hole] == F(0.25)).all() and (od[0][hole] == F(4.0)).all()
    blind, none, _ = fr.fill_holes(img, None, known)
    assert none is None
    print("depth-blind fill of the band: min", blind[0, 0][hole].min(), "max", blind[0, 0][hole].max())
    assert (blind[0, 0][hole] > 0.25).all()
    assert abs(float(blind[0, 0][hole].max()) - 0.77) < 0.01


def test_wrap():
    img = np.zeros((1, 1, 4, 16), F)
    img[..., 8:] = 1.0
    known = np.ones((1, 4, 16), bool)
    known[..., :2] = False
    wrapped, _, _ = fr.fill_holes(img, None, known, None, True)
    plain, _, _ = fr.fill_holes(img, None, known, None, False)
    assert (wrapped[0, 0, :, 0] == F(0.4375)).all()
    assert (plain[0, 0, :, 0] == 0).all()


@pytest.mark.parametrize("levels,left", [(1, 176), (2, 144), (3, 16), (None, 0), (0, 192)])
def test_levels_cap(levels, left):
    img = np.random.default_rng(3).uniform(0, 1, (1, 2, 8, 32)).astype(F)
    known = np.ones((1, 8, 32), bool)
    known[..., 4:28] = False
    out, _, filled = fr.fill_holes(img, None, known, None, False, 0.05, levels)
    unknown = ~known[0] & ~filled[0]
    assert unknown.sum() == left
    assert np.array_equal(bits(out[0][:, unknown]), bits(img[0][:, unknown]))  # what no level reaches keeps its bits


def test_level_sizes():
    assert fr.level_sizes(480, 640) == [(480, 640), (240, 320), (120, 160), (60, 80), (30, 40), (15, 20), (8, 10), (4, 5),
                                        (2, 3), (1, 2), (1, 1)]
    assert fr.level_sizes(7, 10, 2) == [(7, 10), (4, 5), (2, 3)] and fr.level_sizes(1, 1) == [(1, 1)]


def test_domain_and_nan():
    img, dep, known = scene(9, 9, 0.5)
    yy, xx = np.mgrid[:9, :9]
    dom = (yy - 4) ** 2 + (xx - 4) ** 2 <= 16
    out, od, filled = fr.fill_holes(img, dep, known, dom)
    assert not filled[:, ~dom].any()
    assert np.array_equal(bits(out[:, :, ~dom]), bits(img[:, :, ~dom])) and np.array_equal(bits(od[:, ~dom]), bits(dep[:, ~dom]))
    assert np.array_equal(filled[0], dom & ~known[0])
    # a NaN colour of a known pixel propagates into what it fills; the depth stays finite
    img2 = np.zeros((1, 1, 2, 2), F)
    img2[0, 0, 0, 0] = np.nan
    k2 = np.array([[[True, False], [False, False]]])
    o2, _, f2 = fr.fill_holes(img2, None, k2)
    assert np.isnan(o2).all() and f2.sum() == 3


def test_blend():
    S, D, C, H, W = 2, 1, 3, 2, 3
    rng = np.random.default_rng(5)
    img = rng.uniform(0, 1, (S, D, C, H, W)).astype(F)
    dep = np.full((S, D, H, W), 2.0, F)
    dep[1, 0, 0, 0] = np.nan       # pixel (0, 0): layer 0 alone
    dep[0, 0, 0, 1] = 0.0          # pixel (0, 1): layer 1 alone
    dep[1, 0, 0, 2] = 2.2          # pixel (0, 2): layer 1 occluded (2.2 * 0.95 = 2.09 > 2)
    dep[1, 0, 1, 0] = 2.1          # pixel (1, 0): same surface (2.1 * 0.95 = 1.995 <= 2)
    dep[:, 0, 1, 2] = (np.inf, -1.0)  # pixel (1, 2): no layer
    w = np.array([[0.25], [0.75]])
    out, od, cov = fr.blend(img, dep, w, 0.05, fill=-3.0)
    assert np.array_equal(bits(out[0, :, 0, 0]), bits(img[0, 0, :, 0, 0])) and od[0, 0, 0] == 2.0
    assert np.array_equal(bits(out[0, :, 0, 1]), bits(img[1, 0, :, 0, 1]))
    assert np.array_equal(bits(out[0, :, 0, 2]), bits(img[0, 0, :, 0, 2])) and od[0, 0, 2] == 2.0
    for y, x in ((1, 0), (1, 1)):
        want = (F(0.25) * img[0, 0, :, y, x] + F(0.75) * img[1, 0, :, y, x]) / (F(0.25) + F(0.75))
        assert np.array_equal(bits(out[0, :, y, x]), bits(want))
    assert od[0, 1, 1] == 2.0 and od[0, 1, 0] == (F(0.25) * F(2.0) + F(0.75) * F(2.1)) / F(1.0)
    assert (out[0, :, 1, 2] == F(-3.0)).all() and np.isnan(od[0, 1, 2]) and cov[0, 1, 2] == 0
    assert cov.sum() == 5
    # a single layer is the identity wherever it counts, whatever its weight
    one, d1, c1 = fr.blend(img[:1], dep[:1], [0.3], 0.05, fill=7.0)
    ok = c1[0] > 0
    assert np.array_equal(bits(one[0][:, ok]), bits(img[0, 0][:, ok])) and np.array_equal(bits(d1[0][ok]), bits(dep[0, 0][ok]))
