"""numpy fp64 restatement of the radiance-volume contract (include/panonerf_hip.h, "radiance volume"): the brick occupancy
and the ray marcher, once as one plain loop over the lattice and once with the jumps (box faces and unoccupied bricks)
restated.  Vectorised over rays with a loop over k; every operation is written in the header's order, so the two sides
differ only through exp (a few fp64 ulps)."""
import numpy as np

BRICK = 8
SH_C = (0.28209479177387814, 0.48860251190291992, 1.0925484305920792, 0.31539156525252005, 0.54627421529603959)


def sh_basis(u, sh_degree):
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    c0, c1, c2, c3, c4 = SH_C
    cols = [np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c3 * (3.0 * (z * z) - 1.0),
            c2 * (x * z), c4 * (x * x - y * y)]
    return np.stack(cols[:(sh_degree + 1) ** 2], -1)


def bricks(res):
    return tuple((n + BRICK - 2) // BRICK for n in res)


def occupancy(data):
    """uint8 [nbx, nby, nbz]: 1 iff a cell of the brick has a corner with sigma > 0 (a NaN is not > 0)"""
    with np.errstate(invalid="ignore"):
        pos = data[..., 0] > 0
    cell = np.zeros(tuple(n - 1 for n in pos.shape), dtype=bool)
    nx, ny, nz = pos.shape
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                cell |= pos[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk]
    nb = bricks(pos.shape)
    occ = np.zeros(nb, dtype=np.uint8)
    for bi in range(nb[0]):
        for bj in range(nb[1]):
            for bk in range(nb[2]):
                occ[bi, bj, bk] = cell[8 * bi:8 * bi + 8, 8 * bj:8 * bj + 8, 8 * bk:8 * bk + 8].any()
    return occ


def _propose(s, k, n):
    with np.errstate(invalid="ignore"):
        c = np.where(s >= n - 1, n - 1, np.floor(np.where(np.isfinite(s), s, 0.0))).astype(np.int64)
        return np.where(s > k, c, k)


def march(data, lo, step, sh_degree, origins, directions, near, far, march_step, t_min, occ=None, jumps=False):
    """data [nx, ny, nz, C] fp32; lo, step: 3 fp32 values each; rays as fp32 arrays; march_step, t_min fp32 values.
    jumps=False is the plain loop (every lattice point evaluated); jumps=True restates the face jumps and, with an
    occupancy table `occ`, the brick jumps.  Returns fp64 arrays: rgb [R, 3], depth [R], acc [R], attrs [R, E], their
    sums of absolute terms abs_rgb / abs_attrs / abs_wt, `marched` (False: the row wrote zeros and marched nothing),
    `fragile` (a decision within 1e-9 of flipping), `evaluated` (samples whose sigma was interpolated) and `hits` (those
    with sigma > 0)."""
    data = np.asarray(data, dtype=np.float32)
    res = data.shape[:3]
    K = (sh_degree + 1) ** 2
    E = data.shape[3] - 1 - 3 * K
    D64 = data.astype(np.float64).reshape(-1, data.shape[3])
    lo = np.asarray(lo, dtype=np.float32).astype(np.float64)
    st = np.asarray(step, dtype=np.float32).astype(np.float64)
    o = np.asarray(origins, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    R = o.shape[0]
    tn = np.broadcast_to(np.asarray(near, dtype=np.float32).astype(np.float64).reshape(-1), (R,)).copy()
    tf = np.broadcast_to(np.asarray(far, dtype=np.float32).astype(np.float64).reshape(-1), (R,)).copy()
    ms, tmin = float(np.float32(march_step)), float(np.float32(t_min))
    top = np.array([n - 1 for n in res], dtype=np.float64)
    nb = bricks(res)
    with np.errstate(all="ignore"):
        valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & np.isfinite(tn) & np.isfinite(tf)
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        valid &= (ln > 0.0) & (tf > tn)
        ln_s = np.where(valid, ln, 1.0)
        dt = ms / ln_s
        nd = np.ceil((tf - tn) / dt)
        valid &= nd < 2147483648.0
        n = np.where(valid, nd, 0).astype(np.int64)
        stepw = dt * ln_s
        Y = sh_basis(d / ln_s[:, None], sh_degree)

        rgb, acc, wt = np.zeros((R, 3)), np.zeros(R), np.zeros(R)
        attrs, abs_attrs, abs_wt = np.zeros((R, E)), np.zeros((R, E)), np.zeros(R)
        T = np.ones(R)
        fragile = np.zeros(R, dtype=bool)
        evaluated = np.zeros(R, dtype=np.int64)
        hits = np.zeros(R, dtype=np.int64)
        k = np.zeros(R, dtype=np.int64)
        live = valid.copy()

        def coord(kk):
            t = tn + (kk.astype(np.float64) + 0.5) * dt
            return t, ((o + t[:, None] * d) - lo) / st

        def plane(x, p):
            return ((((lo[x] + p * st[x]) - o[:, x]) / d[:, x]) - tn) / dt - 0.5

        while True:
            live &= k < n
            if not live.any():
                break
            t, g = coord(k)
            nxt = k + 1
            fragile |= live & ((np.abs(g) <= 1e-9) | (np.abs(g - top) <= 1e-9)).any(1)
            low, high = ~(g >= 0.0), g > top
            outside = (low | high).any(1)
            if jumps:
                gone = ((low & ~(d > 0.0)) | (high & ~(d < 0.0))).any(1)
                kl = k.copy()
                for x in range(3):
                    for side, p, is_low in ((low[:, x] & (d[:, x] > 0.0), 0.0, True),
                                            (high[:, x] & (d[:, x] < 0.0), top[x], False)):
                        c = _propose(plane(x, p), k, n)
                        for tries in range(2):
                            gc = coord(c)[1][:, x]
                            beyond = ~(gc >= 0.0) if is_low else gc > top[x]
                            c = np.where((c > k) & ~beyond, c - 1 if tries == 0 else k, c)
                        kl = np.where(side & (c > kl), c, kl)
                live &= ~(outside & gone)
                nxt = np.where(outside, kl + 1, nxt)
            inside = live & ~outside
            gi = np.where(inside[:, None], g, 0.0)
            c = np.minimum(np.floor(gi), top - 1.0).astype(np.int64)
            f = gi - c
            if jumps and occ is not None:
                b = c >> 3
                empty = inside & (occ[b[:, 0], b[:, 1], b[:, 2]] == 0)
                s = (n - 1).astype(np.float64)
                for x in range(3):
                    up = np.minimum((b[:, x] + 1) * BRICK, res[x] - 1).astype(np.float64)
                    sx = plane(x, np.where(d[:, x] > 0.0, up, (b[:, x] * BRICK).astype(np.float64)))
                    s = np.where((d[:, x] != 0.0) & (sx < s), sx, s)
                cand = _propose(s, k, n)
                for tries in range(2):
                    gc = coord(cand)[1]
                    inb = (gc >= 0.0) & (gc <= top)
                    cc = np.where(inb, np.minimum(np.floor(np.where(inb, gc, 0.0)), top - 1.0), -BRICK).astype(np.int64)
                    bad = (cand > k) & ~((cc >> 3) == b).all(1)
                    cand = np.where(bad, cand - 1 if tries == 0 else k, cand)
                nxt = np.where(empty, cand + 1, nxt)
                inside &= ~empty
            evaluated += inside
            # the trilinear tap: weights (wx wy) wz, corners in the order i, j, k, low corner first
            tri = np.zeros((R, data.shape[3]))
            for q in range(8):
                qi, qj, qk = q >> 2, (q >> 1) & 1, q & 1
                w = ((f[:, 0] if qi else 1.0 - f[:, 0]) * (f[:, 1] if qj else 1.0 - f[:, 1])) * \
                    (f[:, 2] if qk else 1.0 - f[:, 2])
                v = ((c[:, 0] + qi) * res[1] + (c[:, 1] + qj)) * res[2] + (c[:, 2] + qk)
                tri = tri + w[:, None] * D64[v]
            sigma = tri[:, 0]
            hit = inside & (sigma > 0.0)
            hits += hit
            col = np.zeros((R, 3))
            for kk in range(K):
                col = col + Y[:, kk, None] * tri[:, 1 + 3 * kk:4 + 3 * kk]
            col = np.where(col > 0.0, col, 0.0)
            alpha = 1.0 - np.exp(-sigma * stepw)
            w = np.where(hit, T * alpha, 0.0)
            h = hit[:, None]
            rgb = np.where(h, rgb + w[:, None] * col, rgb)
            a = tri[:, 1 + 3 * K:]
            attrs = np.where(h, attrs + w[:, None] * a, attrs)
            abs_attrs = np.where(h, abs_attrs + w[:, None] * np.abs(a), abs_attrs)
            acc = np.where(hit, acc + w, acc)
            wt = np.where(hit, wt + w * t, wt)
            abs_wt = np.where(hit, abs_wt + w * np.abs(t), abs_wt)
            T = np.where(hit, T * (1.0 - alpha), T)
            if tmin > 0.0:
                fragile |= hit & (np.abs(T - tmin) <= 1e-9 * tmin)
            live &= ~(hit & (T < tmin))
            k = np.where(live, nxt, k)
        q = wt / acc
        q = np.where(np.isnan(q), 0.0, q)
        depth = np.where(valid, np.minimum(np.maximum(q, tn), tf), 0.0)
    return dict(rgb=rgb, depth=depth, acc=acc, attrs=attrs, abs_rgb=rgb.copy(), abs_attrs=abs_attrs, abs_wt=abs_wt,
                marched=valid, fragile=fragile & valid, evaluated=evaluated, hits=hits)


def ulps(got, want64, slack=None):
    """the error of fp32 `got` against fp64 `want64` in fp32 ulps of the rounded reference, after the absolute slack"""
    got = np.asarray(got, dtype=np.float64)
    ref32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    err = np.abs(got - np.asarray(want64, dtype=np.float64))
    if slack is not None:
        err = np.maximum(err - slack, 0.0)
    unit = np.spacing(np.maximum(np.abs(ref32), np.float32(1.1754944e-38))).astype(np.float64)
    return err / unit
