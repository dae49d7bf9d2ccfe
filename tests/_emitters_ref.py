"""fp64 numpy restatement of the emitter contract (include/panonerf_hip.h, pano_nerf_amd.emitters): luminance, the default
threshold, flood-fill labelling under the wrapped 8-neighbourhood, the per-component records and the light a component
stands for; plus the masks and probes the CPU and GPU tests share.  Nothing here imports the package."""
import collections
import math

import numpy as np


# ------------------------------------------------------------------------------------------------------ the probe table
def probe_dirs(H, W):
    """[H W, 3] fp64 unit directions of the probe pixels (lighting.probe_directions' convention: y up, column j looks
    theta = -(j + 1/2) 2 pi / W around it, so column 0 and column W - 1 meet at theta = 0: +z on the equator)"""
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    theta = -(j + 0.5) / W * 2 * np.pi
    phi = (i + 0.5) / H * np.pi
    return np.stack([np.sin(phi) * np.sin(theta), np.cos(phi), np.sin(phi) * np.cos(theta)], -1).reshape(-1, 3)


def probe_omega(H, W):
    y = (np.arange(H) + 0.5) / H
    return (np.sin(y * np.pi)[:, None] * (2 * np.pi / W) * (np.pi / H) * np.ones((1, W))).reshape(-1)


def table(H, W):
    """(dirs, omega) rounded to fp32 as the device holds them (the omegas bit for bit; the directions to a few ulps)"""
    return probe_dirs(H, W).astype(np.float32), probe_omega(H, W).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- conventions
def luminance(probe):
    """[3, H, W] fp32 -> [H, W] fp64: ((double)R + G + B) / 3.0"""
    p = np.asarray(probe, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ((p[0] + p[1]) + p[2]) / 3.0


def threshold(probe, omega, ratio=8.0):
    """fp32: ratio exp(sum omega ln max(Y, 1e-6) / sum omega) over the pixels with finite Y, in pixel order"""
    y = luminance(probe).reshape(-1)
    w = np.asarray(omega, np.float32).astype(np.float64)
    ok = np.isfinite(y)
    num = den = 0.0
    for yy, ww in zip(y[ok], w[ok]):
        num += ww * math.log(max(yy, 1e-6))
        den += ww
    return np.float32(ratio * math.exp(num / den)) if den > 0 else np.float32(np.nan)


def emitter_mask(probe, thr):
    with np.errstate(invalid="ignore"):
        return luminance(probe) > np.float64(np.float32(thr))


def label_mask(mask):
    """(labels int32 [H, W], count): flood fill of a boolean mask under the 8-neighbourhood with column W - 1 next to column
    0 (diagonals across the seam included) and no join across the poles.  The image is scanned in row-major order, so the
    components come out numbered by their smallest pixel index."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    labels = np.full((H, W), -1, np.int32)
    count = 0
    for start in np.flatnonzero(mask.reshape(-1)):
        i0, j0 = divmod(int(start), W)
        if labels[i0, j0] >= 0:
            continue
        labels[i0, j0] = count
        queue = collections.deque([(i0, j0)])
        while queue:
            i, j = queue.popleft()
            for di in (-1, 0, 1):
                ii = i + di
                if ii < 0 or ii >= H:
                    continue
                for dj in (-1, 0, 1):
                    jj = (j + dj) % W
                    if mask[ii, jj] and labels[ii, jj] < 0:
                        labels[ii, jj] = count
                        queue.append((ii, jj))
        count += 1
    return labels, count


def label(probe, thr):
    return label_mask(emitter_mask(probe, thr))


FIELDS = ("pixels", "omega", "flux", "lum_flux", "direction", "peak", "peak_index", "spread", "angular_radius", "distance")


def stats(probe, labels, count, dirs, omega, distance=None):
    """dict of fp64 (int64 for pixels / peak_index) arrays [C, ...]: the record of every component, plus "dir_norm" =
    |sum Y omega d| / lum_flux (the conditioning of `direction`) and "fallback" (the peak pixel's direction was used)"""
    p = np.asarray(probe, np.float32).astype(np.float64).reshape(3, -1)
    y = luminance(probe).reshape(-1)
    d = np.asarray(dirs, np.float32).astype(np.float64)
    w = np.asarray(omega, np.float32).astype(np.float64)
    z = None if distance is None else np.asarray(distance, np.float32).reshape(-1)
    lab = np.asarray(labels).reshape(-1)
    out = {k: [] for k in FIELDS + ("dir_norm", "fallback")}
    for c in range(count):
        pix = np.flatnonzero(lab == c)
        yw = y[pix] * w[pix]
        lum = yw.sum()
        S = (yw[:, None] * d[pix]).sum(0)
        norm = math.sqrt((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2])
        k = int(np.argmax(y[pix]))  # the first of equal maxima: the lowest pixel index
        fallback = not (norm > 0.0 and math.isfinite(norm) and norm >= 1e-12 * lum)
        u = d[pix[k]] if fallback else S / norm
        cross = np.cross(np.broadcast_to(u, d[pix].shape), d[pix])
        ang = np.arctan2(np.sqrt((cross[:, 0] ** 2 + cross[:, 1] ** 2) + cross[:, 2] ** 2),
                         (u[0] * d[pix, 0] + u[1] * d[pix, 1]) + u[2] * d[pix, 2])
        om = w[pix].sum()
        dist = np.nan
        if z is not None:
            with np.errstate(invalid="ignore"):
                ok = (z[pix] > 0) & (z[pix] < np.inf)
            if ok.any():
                dist = (yw[ok] * z[pix][ok].astype(np.float64)).sum() / yw[ok].sum()
        for name, v in (("pixels", len(pix)), ("omega", om), ("flux", (p[:, pix] * w[pix]).sum(1)), ("lum_flux", lum),
                        ("direction", u), ("peak", y[pix[k]]), ("peak_index", int(pix[k])), ("spread", ang.max()),
                        ("angular_radius", math.acos(1.0 - min(om, 4 * math.pi) / (2 * math.pi))), ("distance", dist),
                        ("dir_norm", norm / lum if lum > 0 else 0.0), ("fallback", fallback)):
            out[name].append(v)
    return {k: np.asarray(v) for k, v in out.items()}


def light_of(record, c, probe_position):
    """(position [3], radius, intensity [3]) of component c, from the record rounded to fp32 as the device returns it"""
    f = lambda k: np.asarray(record[k][c], np.float64).astype(np.float32).astype(np.float64)
    dist = float(f("distance"))
    pos = np.asarray(probe_position, np.float64) + f("direction") * dist
    return pos, dist * math.sin(min(float(f("angular_radius")), 0.5 * math.pi)), f("flux") * (dist * dist)


def subset_irradiance(probe, keep, normals, dirs, omega):
    """[K] fp64: the luminance irradiance E(n) = sum_pix Y max(0, n . d) omega over the pixels of the boolean mask keep
    (lighting.irradiance's quadrature on a pixel set)"""
    y = luminance(probe).reshape(-1)
    k = np.asarray(keep, bool).reshape(-1)
    cos = np.asarray(normals, np.float64) @ np.asarray(dirs, np.float64)[k].T
    return (np.where(cos < 0, 0.0, cos) * (y[k] * np.asarray(omega, np.float64)[k])).sum(1)


def energy_gap_and_bound(probe, labels, record, normals, dirs, omega):
    """(|E_all(n) - E_background(n) - sum_i lum_flux_i relu(n . direction_i)| [K], sum_i lum_flux_i 2 sin(spread_i / 2))"""
    lab = np.asarray(labels)
    e_all = subset_irradiance(probe, np.ones_like(lab, bool), normals, dirs, omega)
    e_bg = subset_irradiance(probe, lab < 0, normals, dirs, omega)
    cos = np.asarray(normals, np.float64) @ np.asarray(record["direction"], np.float64).T
    lights = (np.where(cos < 0, 0.0, cos) * np.asarray(record["lum_flux"], np.float64)).sum(1)
    bound = float((np.asarray(record["lum_flux"], np.float64) * 2 * np.sin(np.asarray(record["spread"], np.float64) / 2)).sum())
    return np.abs(e_all - e_bg - lights), bound


# ------------------------------------------------------------------------------------------------- masks for the labels
SIZES = ((2, 2), (2, 3), (3, 2), (5, 7), (8, 16), (33, 65))
THRESHOLD = 1.0  # exactly representable: no rounding of the threshold can move a pixel


def serpentine(H, W):
    """a one-pixel-wide path over the whole image (columns 1 .. W - 2, so it does not close across the seam): every other
    row, joined at alternating ends"""
    m = np.zeros((H, W), bool)
    m[0::2, 1:W - 1] = True
    for i in range(1, H - 1, 2):
        m[i, W - 2 if (i // 2) % 2 == 0 else 1] = True
    return m


def spiral(H, W):
    """a one-pixel-wide rectangular spiral running inwards (columns 1 .. W - 2)"""
    h, w = H, W - 2
    g = np.zeros((h, w), bool)
    i = j = 0
    di, dj = 0, 1
    g[0, 0] = True
    while True:
        moved = False
        for _ in range(2):
            ni, nj, ai, aj = i + di, j + dj, i + 2 * di, j + 2 * dj
            if 0 <= ni < h and 0 <= nj < w and not g[ni, nj] and not (0 <= ai < h and 0 <= aj < w and g[ai, aj]):
                i, j = ni, nj
                g[i, j] = True
                moved = True
                break
            di, dj = dj, -di
        if not moved:
            break
    m = np.zeros((H, W), bool)
    m[:, 1:W - 1] = g
    return m


def comb(H, W):
    """teeth on every other column, joined only by the last row: their provisional labels meet late"""
    m = np.zeros((H, W), bool)
    m[:, 1:W - 1:2] = True
    m[H - 1, 1:W - 1] = True
    return m


def nested_us(H, W):
    """U shapes inside one another, two pixels apart: arms down from row 0, joined at the bottom; one component each"""
    m = np.zeros((H, W), bool)
    k = 0
    while 1 + 2 * k < W - 2 - 2 * k and H - 1 - 2 * k >= 1:
        a, b, bottom = 1 + 2 * k, W - 2 - 2 * k, H - 1 - 2 * k
        m[:bottom + 1, a] = m[:bottom + 1, b] = True
        m[bottom, a:b + 1] = True
        k += 1
    return m


def masks(H, W):
    """name -> boolean [H, W] mask: the patterns that fit the size, and random masks at three densities"""
    out = collections.OrderedDict()
    z = lambda: np.zeros((H, W), bool)
    m = z()
    m[1:min(4, H), [W - 2, W - 1, 0, 1][:min(4, W)]] = True
    out["seam_blob"] = m
    m = z()
    m[0, 0] = m[1, W - 1] = True
    out["seam_diagonal"] = m
    m = z()
    m[H - 1, 0] = m[H - 2, W - 1] = True
    out["seam_antidiagonal"] = m
    if W >= 4:
        m = z()
        m[0, 1] = m[1, 2] = True
        out["diagonal"] = m
        m = z()
        m[0, 0] = m[0, W // 2] = True
        out["row0_opposite"] = m
        m = z()
        m[0, 1] = m[H - 1, 1] = True
        out["pole_to_pole"] = m
    if H >= 5 and W >= 7:
        out["serpentine"], out["spiral"], out["comb"], out["nested_us"] = serpentine(H, W), spiral(H, W), comb(H, W), nested_us(H, W)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out["checkerboard"] = (ii + jj) % 2 == 0
    out["all"], out["none"] = ~z(), z()
    for density in (0.1, 0.4, 0.9):
        for seed in range(3):
            rng = np.random.default_rng([H, W, int(density * 10), seed])
            out[f"random_{density}_{seed}"] = rng.random((H, W)) < density
    return out


def probe_of_mask(mask, seed=0):
    """[3, H, W] fp32 probe whose pixels are above THRESHOLD exactly on the mask (varied values, all finite and >= 0)"""
    rng = np.random.default_rng(seed)
    H, W = mask.shape
    hi = 1.5 + 8.0 * rng.random((3, H, W))
    lo = 0.9 * rng.random((3, H, W))
    return np.where(mask[None], hi, lo).astype(np.float32)


def special_probe():
    """(probe [3, 4, 8], expected emitter mask): NaN, +inf, -inf and exactly-the-threshold pixels among plain ones"""
    p = np.full((3, 4, 8), 0.25, np.float32)
    want = np.zeros((4, 8), bool)
    p[:, 0, 0] = 1.0                       # Y = 1 exactly: not above the threshold
    p[:, 0, 1] = (1.0, 1.0, 1.0000001)     # one ulp above in one channel: Y > 1
    want[0, 1] = True
    p[:, 1, 3] = (np.nan, 9.0, 9.0)        # NaN: no emitter
    p[:, 1, 4] = (np.inf, 0.0, 0.0)        # +inf: an emitter
    want[1, 4] = True
    p[:, 1, 5] = (np.inf, -np.inf, 5.0)    # inf - inf = NaN: no emitter
    p[:, 2, 7] = (-np.inf, 9.0, 9.0)       # -inf: no emitter
    p[:, 3, 0] = 7.0                       # diagonal to (2, 7) across the seam, which is no emitter
    want[3, 0] = True
    p[:, 3, 7] = (np.inf, np.inf, np.inf)  # +inf next to (3, 0) across the seam: one component with it
    want[3, 7] = True
    return p, want


# ------------------------------------------------------------------------------------------------- probes for the records
def blob_probe(H, W, seed=0):
    """(probe [3, H, W], distance [H, W]) fp32: a noisy non-negative ambient below 1 with compact bright blobs (one across the
    seam, one near a pole, a single pixel, two equal peaks in one blob) whose weighted directions barely cancel; the distance
    map holds zeros, an Inf and a NaN inside the blobs.  Emitters are the pixels above THRESHOLD."""
    rng = np.random.default_rng([H, W, seed])
    d = probe_dirs(H, W)
    probe = (0.8 * rng.random((3, H * W))).astype(np.float64)
    axes = np.array([[0.02, 0.25, 1.0], [-1.0, -0.3, 0.2], [0.6, 0.75, -0.3], [0.5, -0.85, -0.5], [1.0, 0.1, 0.1]])
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    radii = (0.45, 0.35, 0.3, 0.4, 0.3)
    for a, r, s in zip(axes, radii, (40.0, 15.0, 25.0, 6.0, 9.0)):
        inside = np.arccos(np.clip(d @ a, -1, 1)) < r
        probe[:, inside] = s * (0.5 + rng.random((3, int(inside.sum()))))
    probe = probe.reshape(3, H, W)
    probe[:, H // 2, W // 3] = (3.0, 2.0, 4.0)  # a single pixel (if it is not inside a blob)
    i, j = np.unravel_index(int(np.argmax(d @ axes[1])), (H, W))
    probe[:, i, j] = 64.0
    probe[:, i, (j + 1) % W] = 64.0  # two equal peaks: the lower index wins
    dist = (1.0 + 4.0 * rng.random((H, W))).astype(np.float32)
    k = np.flatnonzero((probe.mean(0) > THRESHOLD).reshape(-1))
    flat = dist.reshape(-1)
    flat[k[::7]] = 0.0
    flat[k[3]] = np.inf
    flat[k[5]] = np.nan
    flat[k[8]] = -2.0
    return probe.astype(np.float32), dist


def ring_probe(H=16, W=32):
    """[3, H, W] fp32: a closed band of constant radiance around the pole axis, on the two rows next to the equator.  Its
    weighted directions cancel - exactly in exact arithmetic, to about 1e-8 of lum_flux with directions held in fp32 - so
    `direction` is either the peak pixel's (the fallback; every pixel ties, so that is the band's first pixel) or
    ill-conditioned noise."""
    p = np.full((3, H, W), 0.1, np.float32)
    p[:, H // 2 - 1:H // 2 + 1, :] = 5.0
    return p


# ----------------------------------------------------------------------------------------------------- the analytic probe
ANALYTIC = dict(ambient=0.2, radiance=(50.0, 20.0), radius=(0.35, 0.3), distance=(2.0, 3.0),
                axes=((0.05, 0.3, 1.0), (-1.0, -0.4, 0.2)), far=4.0, position=(0.3, -0.2, 0.1))


def analytic_probe(H, W):
    """(probe [3, H, W], distance [H, W], unit axes [2, 3]): an ambient of 0.2 with two discs of radiance 50 and 20 and
    angular radius 0.35 and 0.3 at constant distances 2 and 3; the first disc lies across the seam (its axis is near +z)"""
    a = ANALYTIC
    d = probe_dirs(H, W)
    axes = np.asarray(a["axes"], np.float64)
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    probe = np.empty((3, H * W))
    probe[:] = a["ambient"] * np.array([1.05, 1.0, 0.95])[:, None]
    dist = np.full(H * W, a["far"])
    for ax, rad, r, z in zip(axes, a["radiance"], a["radius"], a["distance"]):
        inside = np.arccos(np.clip(d @ ax, -1, 1)) < r
        probe[:, inside] = rad * np.array([1.1, 1.0, 0.9])[:, None]
        dist[inside] = z
    return probe.reshape(3, H, W).astype(np.float32), dist.reshape(H, W).astype(np.float32), axes


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)
