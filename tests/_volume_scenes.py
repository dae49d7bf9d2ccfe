"""Seeded volumes and ray sets shared by tests/test_volume_cpu.py and tests/test_gpu_volume.py: the smallest grids at
which the marcher can go wrong, and rays of every kind the contract names.  Host numpy only."""
import functools

import numpy as np

BOUNDS = ((-0.503, -0.401, -0.607), (0.611, 0.523, 0.497))

# name -> (resolution, sh_degree, E)
VOLUMES = {
    "one_cell": ((2, 2, 2), 0, 0),
    "strides": ((3, 4, 5), 1, 6),
    "one_brick": ((9, 9, 9), 2, 0),
    "partial": ((10, 9, 17), 2, 6),
    "checker": ((17, 17, 17), 1, 6),
    "single": ((17, 17, 17), 0, 6),
    "nan": ((10, 11, 9), 1, 0),
}
ATTRS = {0: (), 6: (("albedo", 3), ("normal", 3))}


@functools.lru_cache(maxsize=None)
def volume(name):
    """(data fp32 [nx, ny, nz, C], bounds, sh_degree, attributes)"""
    res, deg, E = VOLUMES[name]
    K = (deg + 1) ** 2
    rng = np.random.default_rng(sorted(VOLUMES).index(name) + 11)
    data = rng.standard_normal(res + (1 + 3 * K + E,)).astype(np.float32)
    data[..., 1:4] += 1.5  # a mostly positive base colour; the higher bands push some samples below 0 (the clamp)
    sigma = np.maximum(rng.standard_normal(res) * 12.0 + 6.0, 0.0).astype(np.float32)  # about a third exactly 0
    if name == "checker":  # bricks of 8 cells, (bi + bj + bk) even = full: positive only strictly inside the brick
        i, j, k = np.meshgrid(*[np.arange(17)] * 3, indexing="ij")
        inner = (i % 8 != 0) & (j % 8 != 0) & (k % 8 != 0)
        full = (((i // 8) + (j // 8) + (k // 8)) % 2 == 0) & inner
        sigma = np.where(full, sigma + 1.0, np.where(inner, -np.abs(sigma), 0.0)).astype(np.float32)
    if name == "single":  # one positive vertex at the grid's far corner: the only occupied cell is (15, 15, 15)
        sigma = np.zeros(res, np.float32)
        sigma[16, 16, 16] = 40.0
    if name == "nan":
        sigma[rng.random(res) < 0.1] = np.nan
        sigma[rng.random(res) < 0.2] *= -1.0
        sigma[:9, :9] = np.where(rng.random(res)[:9, :9] < 0.5, np.nan, -1.0)  # brick (0, 0, 0) is empty through NaN and < 0
    data[..., 0] = sigma
    data.setflags(write=False)
    return data, BOUNDS, deg, ATTRS[E]


def placement(bounds, res):
    """geometry._placement: fp32 (lo, step)"""
    lo, hi = bounds
    step = tuple((b - a) / (n - 1) for a, b, n in zip(lo, hi, res))
    return np.array(lo, np.float32), np.array(step, np.float32)


def march_step(bounds, res):
    return np.float32(0.5 * min(float(s) for s in placement(bounds, res)[1]))


@functools.lru_cache(maxsize=None)
def rays(name="mixed", seed=5):
    """dict of fp32 origins [R, 3], directions [R, 3], near [R], far [R] against BOUNDS.  "mixed": rays from inside and
    outside, misses, axis-parallel rays in both signs of all three axes, cell diagonals of every volume above, unnormalised
    directions (|d| from 0.1 to 10) and invalid rows mixed into the valid ones."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(BOUNDS[0]), np.array(BOUNDS[1])
    mid, ext = 0.5 * (lo + hi), hi - lo
    O, D = [], []

    def unit(n):
        v = rng.standard_normal((n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    n = 40  # inside the box
    O.append(lo + rng.random((n, 3)) * ext)
    D.append(unit(n))
    n = 40  # outside, aimed at a point of the box
    o = mid + 1.7 * unit(n)
    O.append(o)
    D.append((lo + rng.random((n, 3)) * ext) - o)
    n = 16  # outside, aimed away or past the box
    o = mid + 1.7 * unit(n)
    O.append(o)
    D.append(np.where(rng.random((n, 1)) < 0.5, o - mid, np.cross(o - mid, unit(n))))
    n = 12  # outside, aimed into the last cell of a 17^3 grid (the single occupied cell of "single")
    o = mid + 1.7 * unit(n)
    O.append(o)
    D.append((hi - rng.random((n, 3)) * ext / 16.0) - o)
    for axis in range(3):  # axis-parallel, both signs, from outside and from inside; the other components exactly 0
        for sign in (1.0, -1.0):
            for start in (-1.3, 0.1):
                for _ in range(3):
                    o = lo + rng.random(3) * ext
                    o[axis] = mid[axis] - sign * (0.5 * ext[axis] + start) + 0.00317
                    d = np.zeros(3)
                    d[axis] = sign
                    O.append(o[None])
                    D.append(d[None])
    for res, _, _ in VOLUMES.values():  # along cell diagonals, through vertices; the start is off the lattice
        step = ext / (np.array(res) - 1)
        for sx in (1.0, -1.0):
            sgn = np.array([sx, 1.0, -sx])
            c = lo + step * np.floor(rng.random(3) * (np.array(res) - 1))
            O.append((c - 2.137 * sgn * step)[None])
            D.append((sgn * step / np.linalg.norm(step))[None])
    O, D = np.concatenate(O), np.concatenate(D)
    R = O.shape[0]
    scale = np.exp(rng.uniform(np.log(0.1), np.log(10.0), R))  # |d| from 0.1 to 10
    scale[rng.random(R) < 0.3] = 1.0
    D = D / np.linalg.norm(D, axis=1, keepdims=True) * scale[:, None]
    near = np.where(rng.random(R) < 0.5, 0.0, rng.uniform(0.0, 0.4, R)) / scale
    far = rng.uniform(2.6, 3.4, R) / scale
    # invalid rows mixed in: NaN / Inf / zero length / far <= near
    for row, what in zip(rng.choice(R, 10, replace=False), range(10)):
        if what == 0:
            O[row, 1] = np.nan
        elif what == 1:
            D[row, 2] = np.inf
        elif what == 2:
            D[row] = 0.0
        elif what == 3:
            far[row] = near[row]
        elif what == 4:
            far[row] = near[row] - 1.0
        elif what == 5:
            near[row] = np.nan
        elif what == 6:
            far[row] = np.inf
        elif what == 7:
            O[row, 0] = -np.inf
        elif what == 8:
            D[row, 0] = np.nan
        else:
            D[row] = -0.0
    out = dict(origins=O.astype(np.float32), directions=D.astype(np.float32), near=near.astype(np.float32),
               far=far.astype(np.float32))
    for v in out.values():
        v.setflags(write=False)
    return out


# camera frames: name -> (constructor name in pano_nerf_amd.views, arguments); the pose keeps lattice points off the faces
CAMERAS = {
    "pano": ("pano_camera", (16, 32)),
    "pinhole": ("perspective_camera", (12, 16, 14.0)),
    "cube": ("cubemap_camera", (4,)),
    "fisheye": ("fisheye_camera", (16, 16)),
    "stereo": ("stereo_pano_camera", (8, 16, 0.064, "left")),
}
CAMERA_NEAR, CAMERA_FAR = 0.0, 2.5


def camera_pose():
    a, b = 0.37, -0.21
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx
    m[:3, 3] = (0.0131, -0.0217, 0.0373)
    return m.astype(np.float32)
