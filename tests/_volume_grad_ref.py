"""numpy fp64 restatement of the marcher's reverse sweep (include/panonerf_hip.h, "radiance volume: gradients"), on the
plain lattice loop of tests/_volume_ref.py (no jumps: they skip samples that add nothing).  Vectorised over rays with a
loop over k; every operation is written in the header's order, so the device differs only through exp (a few fp64
ulps) and the quantisation.  Host numpy only."""
import numpy as np

import _volume_ref as ref

QUANTUM = 2.0 ** -40


class Sweep:
    """The rows of one march call and the loop over their compositing samples.  data is rounded to fp32 as the device
    sees it, unless exact=True (fp64 data taken as given: what a central difference perturbs)."""

    def __init__(self, data, lo, step, sh_degree, origins, directions, near, far, march_step, t_min, exact=False):
        data = np.asarray(data, dtype=np.float64) if exact else np.asarray(data, dtype=np.float32)
        self.res = data.shape[:3]
        self.C = data.shape[3]
        self.K = (sh_degree + 1) ** 2
        self.Cg = 1 + 3 * self.K
        self.D64 = data.astype(np.float64).reshape(-1, self.C)
        self.lo = np.asarray(lo, dtype=np.float32).astype(np.float64)
        self.st = np.asarray(step, dtype=np.float32).astype(np.float64)
        self.o = np.asarray(origins, dtype=np.float32).astype(np.float64).reshape(-1, 3)
        self.d = np.asarray(directions, dtype=np.float32).astype(np.float64).reshape(-1, 3)
        R = self.R = self.o.shape[0]
        self.tn = np.broadcast_to(np.asarray(near, dtype=np.float32).astype(np.float64).reshape(-1), (R,)).copy()
        self.tf = np.broadcast_to(np.asarray(far, dtype=np.float32).astype(np.float64).reshape(-1), (R,)).copy()
        ms, self.tmin = float(np.float32(march_step)), float(np.float32(t_min))
        o, d, tn, tf = self.o, self.d, self.tn, self.tf
        with np.errstate(all="ignore"):
            valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & np.isfinite(tn) & np.isfinite(tf)
            ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            valid &= (ln > 0.0) & (tf > tn)
            ln_s = np.where(valid, ln, 1.0)
            self.dt = ms / ln_s
            nd = np.ceil((tf - tn) / self.dt)
            valid &= nd < 2147483648.0
            self.n = np.where(valid, nd, 0).astype(np.int64)
            self.stepw = self.dt * ln_s
            self.Y = ref.sh_basis(d / ln_s[:, None], sh_degree)
        self.valid = valid
        self.fragile = np.zeros(R, dtype=bool)

    def samples(self):
        """Yields, for k = 0, 1, ..: dict of hit [R] (the sample composites), inside [R] (its sigma was interpolated), v
        [R, 8] corner vertices, w [R, 8] corner weights, sigma [R], s [R, 3] the unclamped colour sums, alpha, wgt (0
        where not hit), T (before the sample) and t."""
        R, res, K = self.R, self.res, self.K
        top = np.array([n - 1 for n in res], dtype=np.float64)
        T = np.ones(R)
        live = self.valid.copy()
        with np.errstate(all="ignore"):
            for k in range(int(self.n.max()) if R else 0):
                live = live & (k < self.n)
                if not live.any():
                    break
                t = self.tn + (float(k) + 0.5) * self.dt
                g = ((self.o + t[:, None] * self.d) - self.lo) / self.st
                self.fragile |= live & ((np.abs(g) <= 1e-9) | (np.abs(g - top) <= 1e-9)).any(1)
                outside = (~(g >= 0.0) | (g > top)).any(1)
                inside = live & ~outside
                gi = np.where(inside[:, None], g, 0.0)
                c = np.minimum(np.floor(gi), top - 1.0).astype(np.int64)
                f = gi - c
                w = np.zeros((R, 8))
                v = np.zeros((R, 8), dtype=np.int64)
                tri = np.zeros((R, self.C))
                for q in range(8):
                    qi, qj, qk = q >> 2, (q >> 1) & 1, q & 1
                    w[:, q] = ((f[:, 0] if qi else 1.0 - f[:, 0]) * (f[:, 1] if qj else 1.0 - f[:, 1])) * \
                        (f[:, 2] if qk else 1.0 - f[:, 2])
                    v[:, q] = ((c[:, 0] + qi) * res[1] + (c[:, 1] + qj)) * res[2] + (c[:, 2] + qk)
                    tri = tri + w[:, q, None] * self.D64[v[:, q]]
                sigma = tri[:, 0]
                hit = inside & (sigma > 0.0)
                s = np.zeros((R, 3))
                for kk in range(K):
                    s = s + self.Y[:, kk, None] * tri[:, 1 + 3 * kk:4 + 3 * kk]
                alpha = 1.0 - np.exp(-sigma * self.stepw)
                wgt = np.where(hit, T * alpha, 0.0)
                yield dict(hit=hit, inside=inside, v=v, w=w, sigma=sigma, s=s, alpha=alpha, wgt=wgt, T=T.copy(), t=t)
                T = np.where(hit, T * (1.0 - alpha), T)
                if self.tmin > 0.0:
                    self.fragile |= hit & (np.abs(T - self.tmin) <= 1e-9 * self.tmin)
                live = live & ~(hit & (T < self.tmin))


def _upstream(R, g_rgb, g_acc):
    g = np.zeros((R, 3)) if g_rgb is None else np.asarray(g_rgb, dtype=np.float32).astype(np.float64).reshape(R, 3)
    ga = np.zeros(R) if g_acc is None else np.asarray(g_acc, dtype=np.float32).astype(np.float64).reshape(R)
    return g, ga


def _u(smp, g, ga):
    col = np.where(smp["s"] > 0.0, smp["s"], 0.0)
    return ((g[:, 0] * col[:, 0] + g[:, 1] * col[:, 1]) + g[:, 2] * col[:, 2]) + ga


def forward(sweep, g_rgb=None, g_acc=None):
    """Pass 1: dict of rgb [R, 3], acc [R] (the forward's sums, term for term), U [R] = sum wgt u, and abs_u [R], the sum
    of |g_c| wgt col_c + |g_a| wgt: what fp64 round-off of U is measured against."""
    R = sweep.R
    g, ga = _upstream(R, g_rgb, g_acc)
    rgb, acc, U, abs_u = np.zeros((R, 3)), np.zeros(R), np.zeros(R), np.zeros(R)
    with np.errstate(all="ignore"):
        for smp in sweep.samples():
            hit, wgt = smp["hit"], smp["wgt"]
            col = np.where(smp["s"] > 0.0, smp["s"], 0.0)
            rgb = np.where(hit[:, None], rgb + wgt[:, None] * col, rgb)
            acc = np.where(hit, acc + wgt, acc)
            U = np.where(hit, U + wgt * _u(smp, g, ga), U)
            abs_u = np.where(hit, abs_u + wgt * ((np.abs(g) * col).sum(1) + np.abs(ga)), abs_u)
    return dict(rgb=rgb, acc=acc, U=U, abs_u=abs_u)


def quantise(x, quantum):
    """(m int64, bad): m = rint(x / quantum), half to even; bad where x is not finite or |x / quantum| >= 2^52 (m = 0)"""
    with np.errstate(all="ignore"):
        xq = x / quantum
        bad = ~(np.abs(xq) < 2.0 ** 52)
        return np.where(bad, 0.0, np.rint(np.where(bad, 0.0, xq))).astype(np.int64), bad


def march_grad(data, lo, step, sh_degree, origins, directions, near, far, march_step, t_min, g_rgb=None, g_acc=None,
               quantum=None, exact=False):
    """The reverse sweep.  Returns dict of grad fp64 [N, 1 + 3 K] (the sum of the contributions), count int64 [N, 1 + 3 K]
    (how many were written), abs [N, 1 + 3 K] (the sum of their absolute values), pass 1's rgb / acc / U / abs_u, marched
    and fragile [R] as tests/_volume_ref.march has them and, with a quantum, sums int64 [N, 1 + 3 K] and flag."""
    sw = Sweep(data, lo, step, sh_degree, origins, directions, near, far, march_step, t_min, exact)
    R, K, Cg = sw.R, sw.K, sw.Cg
    N = sw.D64.shape[0]
    g, ga = _upstream(R, g_rgb, g_acc)
    fwd = forward(sw, g_rgb, g_acc)
    U = fwd["U"]
    grad, count, tot = np.zeros((N, Cg)), np.zeros((N, Cg), dtype=np.int64), np.zeros((N, Cg))
    sums, flag = np.zeros((N, Cg), dtype=np.int64), False

    P = np.zeros(R)
    chan = np.arange(Cg)
    with np.errstate(all="ignore"):
        for smp in sw.samples():
            hit, wgt, w, v, s = smp["hit"], smp["wgt"], smp["w"], smp["v"], smp["s"]
            if not hit.any():
                continue
            u = _u(smp, g, ga)
            P = np.where(hit, P + wgt * u, P)
            Tn = smp["T"] * (1.0 - smp["alpha"])
            ds = sw.stepw * (Tn * u - (U - P))
            # the contributions x [R, 8, 1 + 3 K] of this sample and which of them are written
            x = np.zeros((R, 8, Cg))
            made = np.zeros((R, 8, Cg), dtype=bool)
            x[:, :, 0] = w * ds[:, None]
            made[:, :, 0] = hit[:, None]
            for kk in range(K):
                for ch in range(3):
                    x[:, :, 1 + 3 * kk + ch] = w * (sw.Y[:, kk] * (wgt * g[:, ch]))[:, None]
                    made[:, :, 1 + 3 * kk + ch] = (hit & (s[:, ch] > 0.0))[:, None]
            at = (v[:, :, None] * Cg + chan)[made]
            xs = x[made]
            np.add.at(grad.reshape(-1), at, xs)
            np.add.at(count.reshape(-1), at, 1)
            np.add.at(tot.reshape(-1), at, np.abs(xs))
            if quantum is not None:
                m, bad = quantise(xs, quantum)
                np.add.at(sums.reshape(-1), at, m)
                flag = flag or bool(bad.any())
    out = dict(grad=grad, count=count, abs=tot, marched=sw.valid, fragile=sw.fragile & sw.valid, **fwd)
    if quantum is not None:
        out.update(sums=sums, flag=flag)
    return out


def near_gate(data, lo, step, sh_degree, origins, directions, near, far, march_step, t_min, margin):
    """bool [N]: vertices that carry weight in a sample whose sigma, or (if it composites) one of whose unclamped colour
    sums, lies within `margin` of its gate at 0: there a difference quotient straddles a kink"""
    sw = Sweep(data, lo, step, sh_degree, origins, directions, near, far, march_step, t_min, exact=True)
    out = np.zeros(sw.D64.shape[0], dtype=bool)
    for smp in sw.samples():
        close = smp["inside"] & (np.abs(smp["sigma"]) <= margin)
        close |= smp["hit"] & (np.abs(smp["s"]) <= margin).any(1)
        touched = close[:, None] & (smp["w"] > 0.0)
        out[smp["v"][touched]] = True
    return out
