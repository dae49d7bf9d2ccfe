"""Volumes and rays for the sparse radiance volume (tests/test_sparse_volume_cpu.py, tests/test_gpu_sparse_volume.py): the
seven scenes of tests/_volume_scenes.py, unchanged, plus three that aim at the brick pool.  Host numpy only.

    corner   17^3, ONE positive vertex, at (8, 8, 8): eight present bricks through one shared vertex, so every one of the
             eight stored copies must agree
    gap      25 x 10 x 9: three bricks along x with the middle one absent (its vertices are <= 0 with live colour), and
             partial bricks (10 vertices along y: a second brick of one cell); rays along x and diagonals that go
             present -> absent -> present are added to the shared set
    tiny16   10 x 9 x 9 with the values at which fp16 rounding can go wrong, and a brick whose only positive sigma, 2e-8,
             rounds to 0 in fp16 (present in the sparse form, unoccupied in its dense expansion)"""
import functools

import numpy as np

import _volume_scenes as base

BOUNDS = base.BOUNDS
EXTRA = {
    "corner": ((17, 17, 17), 1, 6),
    "gap": ((25, 10, 9), 1, 0),
    "tiny16": ((10, 9, 9), 0, 0),
}
NAMES = sorted(base.VOLUMES) + sorted(EXTRA)

TIE_DOWN = np.float32(1.0 + 2.0 ** -11)      # half way between 1 and 1 + 2^-10: to the even 1
TIE_UP = np.float32(1.0 + 3.0 * 2.0 ** -11)  # half way between 1 + 2^-10 and 1 + 2^-9: to the even 1 + 2^-9


@functools.lru_cache(maxsize=None)
def volume(name):
    """(data fp32 [nx, ny, nz, C], bounds, sh_degree, attributes)"""
    if name in base.VOLUMES:
        return base.volume(name)
    res, deg, E = EXTRA[name]
    K = (deg + 1) ** 2
    rng = np.random.default_rng(sorted(EXTRA).index(name) + 101)
    data = rng.standard_normal(res + (1 + 3 * K + E,)).astype(np.float32)
    data[..., 1:4] += 1.5
    sigma = np.maximum(rng.standard_normal(res) * 12.0 + 6.0, 0.0).astype(np.float32)
    if name == "corner":
        sigma = np.where(rng.random(res) < 0.5, 0.0, -np.abs(sigma) - 1.0).astype(np.float32)
        sigma[8, 8, 8] = 40.0
    if name == "gap":
        sigma[8:17] = -np.abs(sigma[8:17])  # the faces i = 8 and i = 16 are shared with the present bricks
    if name == "tiny16":
        sigma[8:] = -np.abs(sigma[8:])
        sigma[9, 4, 4] = 2e-8              # alone in brick (1, 0, 0): present, and 0 in fp16
        sigma[1, 1, 1] = 1e-6              # a half subnormal
        sigma[1, 1, 2] = 3e-8              # just above half the smallest half subnormal: rounds up to it
        sigma[1, 1, 3] = 2.9e-8            # just below: rounds to 0
        sigma[1, 2, 1] = 65504.0           # the largest half
        sigma[1, 2, 2] = TIE_DOWN
        sigma[1, 2, 3] = TIE_UP
        sigma[1, 3, 1] = 1e-40             # an fp32 subnormal
        data[2, 1, 1, 1:] = (65504.0, -65504.0, 1e-6)
        data[2, 1, 2, 1:] = (TIE_DOWN, -TIE_UP, -3e-8)
        data[2, 1, 3, 1:] = (1e-40, -1e-40, 2.9e-8)
        data[2, 2, 1, 1:] = (-0.0, 6.104e-5, 6.0e-5)  # the smallest normal half, 2^-14 = 6.1035e-5, and just below it
    data[..., 0] = sigma
    data.setflags(write=False)
    return data, BOUNDS, deg, base.ATTRS[E]


@functools.lru_cache(maxsize=None)
def half_volume(name):
    """volume(name) with every value rounded to fp16 and widened again: what fp16 storage holds (none overflows)"""
    data, bounds, deg, attrs = volume(name)
    with np.errstate(over="raise"):
        out = data.astype(np.float16).astype(np.float32)
    out.setflags(write=False)
    return out, bounds, deg, attrs


def _gap_rays():
    """along x in both senses and along diagonals, from outside the box, through present -> absent -> present bricks"""
    rng = np.random.default_rng(23)
    lo, hi = np.array(BOUNDS[0]), np.array(BOUNDS[1])
    ext = hi - lo
    O, D = [], []
    for sign in (1.0, -1.0):
        for _ in range(6):  # axis-parallel: y and z anywhere in the box (both y bricks), the other components exactly 0
            o = lo + rng.random(3) * ext
            o[0] = (lo[0] - 0.31) if sign > 0 else (hi[0] + 0.29)
            O.append(o)
            D.append(np.array([sign, 0.0, 0.0]))
        for _ in range(6):  # diagonals that enter through one x face and leave through the other
            a, b = lo + rng.random(3) * ext, lo + rng.random(3) * ext
            a[0], b[0] = (lo[0], hi[0]) if sign > 0 else (hi[0], lo[0])
            d = (b - a) / np.linalg.norm(b - a)
            O.append(a - 0.37 * d)
            D.append(d * rng.uniform(0.3, 3.0))
    O, D = np.array(O), np.array(D)
    ln = np.linalg.norm(D, axis=1)
    return dict(origins=O.astype(np.float32), directions=D.astype(np.float32), near=np.zeros(len(O), np.float32),
                far=(3.1 / ln).astype(np.float32))


@functools.lru_cache(maxsize=None)
def rays(name):
    """the shared ray set of _volume_scenes.rays(); for "gap" with the rays through its absent brick appended"""
    r = base.rays()
    if name != "gap":
        return r
    extra = _gap_rays()
    out = {k: np.concatenate([r[k], extra[k]]) for k in r}
    for v in out.values():
        v.setflags(write=False)
    return out


placement = base.placement
march_step = base.march_step


def big_step(name):
    data, bounds, _, _ = volume(name)
    return np.float32(2.7 * max(placement(bounds, data.shape[:3])[1]))
