"""fp64 restatements of the sampling and encoding kernels of pn_render.hip (k_sample_coarse, k_sample_env, k_resample,
k_ipe_encode, k_pos_enc_view, k_lit_rays), written from oracle/pano_oracle.py (cast_rays, _jitter, sample_along_rays,
sample_each_points, piecewise_constant_pdf, resample_along_rays, integrated_pos_enc, pos_enc, generate_lit_rays) and
evaluated in fp64 on the fp32 input values.  Where the operation itself contains an fp32 rounding the restatement keeps
it and does the rest in fp64: the torch.linspace grid, u = s * fl32(1 / S) + u_rand clamped to 1 - eps32, the encoding
arguments fl32(mean * 2^l), fl32(y + fl32(pi / 2)) and fl32(cov * 4^l), and the surface point x_surf = origins +
directions * distance that sample_each_points receives as an fp32 input.

Every criterion is per element and in a conditioning unit (never at tensor scale):
  mean          eps32 * (|d_c| * t_mean + |o_c|)
  cov           eps32 * (|t_var| * d_c^2 + r_var)       (r_var without the null factor: 1 - d^2 / |d|^2 cancels to ~eps32)
  coarse/env t  eps32 * max(|lower|, |upper|, |t|), with disparity eps32 * |t|
  resampled t   the fp64 inverse CDF at u - DELTA, u, u + DELTA brackets the value (resample_bracket)
  encodings     eps32 * exp(-v / 2) + 2^-126

Also the input suites that test_sampling_ref_cpu.py and test_gpu_sampling.py share."""
import functools

import numpy as np
import torch

from oracle import pano_oracle as orc

f32 = np.float32
EPS32 = 2.0 ** -23
TINY32 = 2.0 ** -126
ONE_M = 1.0 - EPS32                   # the largest u / the largest uniform used
DELTA = 16 * EPS32                    # resampling: twice the ~8 eps32 of absolute error a 512-bin fp32 CDF can carry
MEAN_UNITS, COV_UNITS = 8.0, 16.0     # cone -> Gaussian: 4 x the fp32 oracle's own 1.6 / 4.35 units, rounded
WIDE_REL, WIDE_SHARE_CAP = 1e-4, 0.05  # at most 5 % of a case's brackets wider than 1e-4 of the ray
T_FLOOR_UNITS = 4.0                   # coarse / env t: 4 x the oracle's own figure, never below 4 units
ENC_FLOOR_UNITS = 4.0                 # encodings: the larger of 4 units and twice the device's own sin / exp


def D(x):
    return torch.as_tensor(x).double()


def units(got, ref, unit):
    """max over the elements of |got - ref| / unit (an exact element counts 0 whatever its unit)."""
    err = (D(got) - D(ref)).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / D(unit).clamp(min=1e-300))
    assert not torch.isnan(D(ref)).any(), "the reference itself is NaN: the input holds a 0/0 interval"
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------- cone -> Gaussian
def cast_rays64(t, origins, directions, radii):
    """orc.cast_rays in fp64.  t [R, S]; origins, directions [R, 3]; radii [R] or [R, 1].
    -> mean, cov [R, S - 1, 3] and their units."""
    t, o, d, r = D(t), D(origins), D(directions), D(radii).reshape(-1, 1)
    t0, t1 = t[:, :-1], t[:, 1:]
    mu, hw = (t0 + t1) / 2, (t1 - t0) / 2
    den = 3 * mu ** 2 + hw ** 2
    t_mean = mu + (2 * mu * hw ** 2) / den
    t_var = hw ** 2 / 3 - (4 / 15) * ((hw ** 4 * (12 * mu ** 2 - hw ** 2)) / den ** 2)
    r_var = r ** 2 * (mu ** 2 / 4 + (5 / 12) * hw ** 2 - (4 / 15) * hw ** 4 / den)
    d2 = d ** 2
    null = 1 - d2 / (d2.sum(-1, keepdim=True) + 1e-10)
    mean = d[:, None, :] * t_mean[..., None] + o[:, None, :]
    cov = t_var[..., None] * d2[:, None, :] + r_var[..., None] * null[:, None, :]
    umean = EPS32 * (d.abs()[:, None, :] * t_mean.abs()[..., None] + o.abs()[:, None, :])
    ucov = EPS32 * (t_var.abs()[..., None] * d2[:, None, :] + r_var[..., None].expand(-1, -1, 3))
    return mean, cov, umean, ucov


def zero_intervals(t):
    """number of intervals with t0 = t1 = 0, where the stable-cone formula is 0/0 (in fp64 too)."""
    t = D(t)
    return int(((t[:, :-1] == 0) & (t[:, 1:] == 0)).sum())


# ------------------------------------------------------------------------------------------------- coarse and env t
def coarse_t64(near, far, N, t_rand=None, disparity=False):
    """orc.sample_along_rays' t in fp64 on the fp32 linspace grid.  near, far [R]; t_rand [R, N + 1] or [1, N + 1] or None.
    -> t [R, N + 1] and its unit."""
    x = torch.linspace(0.0, 1.0, N + 1).double()
    nr, fr = D(near).reshape(-1, 1), D(far).reshape(-1, 1)
    if disparity:
        t = 1.0 / (1.0 / nr * (1.0 - x) + 1.0 / fr * x)
    else:
        t = nr + (fr - nr) * x
    scale = t.abs()
    if t_rand is not None:
        mids = 0.5 * (t[:, 1:] + t[:, :-1])
        upper = torch.cat([mids, t[:, -1:]], -1)
        lower = torch.cat([t[:, :1], mids], -1)
        t = lower + (upper - lower) * D(t_rand)
        scale = t.abs() if disparity else torch.maximum(torch.maximum(lower.abs(), upper.abs()), t.abs())
    return t, EPS32 * scale


def surface_points32(origins, directions, distance):
    """x_surf as the fp32 callers of sample_each_points form it (two roundings, no contraction)."""
    return origins + directions * distance.view(-1, 1)


def env_expand(x_surf, env_dirs, env_radii, env_near, env_far):
    """per light ray r = b * D + j: origin, direction, radius, near, far (orc.sample_each_points' expansion)."""
    B, Dn = x_surf.shape[0], env_dirs.shape[0]
    o = x_surf[:, None, :].expand(B, Dn, 3).reshape(-1, 3)
    d = env_dirs[None].expand(B, Dn, 3).reshape(-1, 3)
    rep = lambda a: a.reshape(1, Dn).expand(B, Dn).reshape(-1)
    return o, d, rep(env_radii), rep(env_near), rep(env_far)


# ------------------------------------------------------------------------------------------------- resampling
def blur(w):
    wp = torch.cat([w[:, :1], w, w[:, -1:]], -1)
    wm = torch.maximum(wp[:, :-1], wp[:, 1:])
    return 0.5 * (wm[:, :-1] + wm[:, 1:])


def cdf64(weights, padding):
    """the CDF of orc.resample_along_rays + piecewise_constant_pdf in fp64; padding enters as its fp32 value."""
    w = D(weights)
    B, N = w.shape
    bl = blur(w) + float(f32(padding))
    ws = bl.sum(-1, keepdim=True)
    pad = torch.clamp(1e-5 - ws, min=0)
    pdf = (bl + pad / N) / (ws + pad)
    cdf = torch.clamp(torch.cumsum(pdf[:, :-1], -1), max=1.0)
    z = torch.zeros(B, 1, dtype=torch.float64)
    return torch.cat([z, cdf, z + 1], -1)


def u32(B, S, u_rand=None):
    """the fp32 sample positions: torch.linspace(0, 1 - eps32, S), or fl32(fl32(s * fl32(1 / S)) + u_rand) clamped."""
    if u_rand is None:
        return torch.linspace(0.0, ONE_M, S).expand(B, S).contiguous()
    u = torch.arange(S, dtype=torch.float32)[None] * float(f32(1.0 / S)) + u_rand
    return torch.clamp(u, max=ONE_M).contiguous()


def inverse_cdf(cdf, bins, u):
    """searchsorted from the right, the den < 1e-5 -> 1 rule and the interpolation, in the dtype of the arguments."""
    S = cdf.shape[1]
    idx = torch.searchsorted(cdf, u.contiguous(), right=True)
    lo, hi = (idx - 1).clamp(min=0), idx.clamp(max=S - 1)
    c0, c1 = cdf.gather(-1, lo), cdf.gather(-1, hi)
    b0, b1 = bins.gather(-1, lo), bins.gather(-1, hi)
    den = c1 - c0
    den = torch.where(den < 1e-5, torch.ones_like(den), den)
    return b0 + (u - c0) / den * (b1 - b0)


def resample_bracket(bins, weights, padding, u):
    """[lo, hi] of the fp64 inverse CDF at u - DELTA, u, u + DELTA (clamped to [0, 1]) and the absolute tolerance
    4 eps32 max |bins|: inside an ordinary bin that is +- DELTA / den * bw, the conditioning; at a knot where the inverse
    jumps (a den < 1e-5 bin, a plateau within an ulp of 1 under the last u) it spans the jump."""
    c, b, u = cdf64(weights, padding), D(bins), D(u)
    vals = [inverse_cdf(c, b, uu) for uu in ((u - DELTA).clamp(min=0.0), u, (u + DELTA).clamp(max=1.0))]
    lo = torch.minimum(torch.minimum(vals[0], vals[1]), vals[2])
    hi = torch.maximum(torch.maximum(vals[0], vals[1]), vals[2])
    return lo, hi, 4 * EPS32 * float(b.abs().max())


def bracket_excess(t, lo, hi, tol):
    """(number of samples outside [lo - tol, hi + tol], the worst distance outside in units of tol)."""
    t = D(t)
    out = torch.maximum(lo - t, t - hi).clamp(min=0)
    out = torch.where(torch.isnan(t), torch.full_like(out, float("inf")), out)
    return int((out > tol).sum()), float(out.max() / tol)


def wide_share(lo, hi, bins):
    """share of the samples whose bracket is wider than WIDE_REL of the ray: what the criterion cannot see."""
    b = D(bins)
    return float(((hi - lo) > WIDE_REL * (b[:, -1:] - b[:, :1])).double().mean())


# ------------------------------------------------------------------------------------------------- encodings
def ipe64(mean, cov):
    """orc.integrated_pos_enc(., ., 0, 16) in fp64 on the fp32 arguments -> enc [M, 96], its unit, the fp32 arguments."""
    sc = torch.tensor([2.0 ** i for i in range(16)])
    y = (mean[:, None, :] * sc[:, None]).flatten(-2)
    v = (cov[:, None, :] * sc[:, None] ** 2).flatten(-2)
    y2 = torch.cat([y, y + orc.HALF_PI_F32], -1)
    v2 = torch.cat([v, v], -1)
    assert y2.dtype == torch.float32 and v2.dtype == torch.float32
    e = torch.exp(-0.5 * v2.double())
    return e * torch.sin(y2.double()), EPS32 * e + TINY32, y2, v2


def view_enc64(x):
    """orc.pos_enc(., 0, 4) in fp64 on the fp32 arguments -> [R, 27] (identity first), the unit, the fp32 arguments."""
    sc = torch.tensor([2.0 ** i for i in range(4)])
    xb = (x[:, None, :] * sc[:, None]).flatten(-2)
    y2 = torch.cat([xb, xb + orc.HALF_PI_F32], -1)
    assert y2.dtype == torch.float32
    ref = torch.cat([x.double(), torch.sin(y2.double())], -1)
    return ref, torch.full_like(ref, EPS32 + TINY32), y2


# ------------------------------------------------------------------------------------------------- light rays
def lit_rays64(num, radius, near, far):
    """orc.generate_lit_rays before its rounding to fp16, in pn_lit_rays' layout: origins, directions, viewdirs [D, 3],
    radii, lossmult, near, far, noise_var [D] -> [14 D] fp64."""
    ga = np.pi * (3.0 - np.sqrt(5.0))
    i = np.arange(num, dtype=np.float64)
    y = 1 - (i / float(num - 1)) * 2
    r = np.sqrt(1 - y * y)
    th = ga * i
    d = np.stack([np.cos(th) * r, y, np.sin(th) * r], -1)
    v = d / np.linalg.norm(d, axis=-1, keepdims=True)
    one = np.ones(num)
    return np.concatenate([np.zeros(3 * num), d.reshape(-1), v.reshape(-1), float(radius) * one, (4 * np.pi / num) * one,
                           near * one, far * one, 0 * one])


def lit_rays_oracle_bits(num, radius, near, far):
    rays = orc.generate_lit_rays(num, radius, near, far)
    return np.concatenate([getattr(rays, k).numpy().reshape(-1) for k in orc.Rays._fields]).view(np.uint16)


def near_half_tie(x):
    """elements of the fp64 array x within 2^-40 relative of the midpoint of two neighbouring fp16 values: the only
    places where two correct fp64 evaluations may round to different halves."""
    x = np.asarray(x, dtype=np.float64)
    h = x.astype(np.float16)
    up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    h = h.astype(np.float64)
    dist = np.minimum(np.abs(x - 0.5 * (h + up)), np.abs(x - 0.5 * (h + dn)))
    return dist <= 2.0 ** -40 * np.abs(x)


def half_ulps_apart(a_bits, b_bits):
    """distance of two fp16 bit patterns in units of the last place (sign-magnitude -> ordered integers)."""
    def key(u):
        u = u.astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7fff), u & 0x7fff)
    return np.abs(key(np.asarray(a_bits)) - key(np.asarray(b_bits)))


# ------------------------------------------------------------------------------------------------- input suites
def _unit(g, n):
    d = torch.randn(n, 3, generator=g)
    return d / d.norm(dim=-1, keepdim=True)


def _direction_pool(g):
    """unit, +-axes, near-axis, fp16-rounded and zero directions."""
    u = _unit(g, 3)
    return torch.stack([u[0], torch.tensor([0., 0., 1.]), torch.tensor([1e-4, 0., 1.]), torch.zeros(3),
                        torch.tensor([0., -1., 0.]), u[1].half().float(), torch.tensor([-1., 0., 0.]), u[2]])


COARSE_SHAPES = [(1, 1), (5, 2), (3, 33), (5, 64), (3, 512)]  # 5 x 64 and 3 x 512 cross a 256-thread block inside a ray


@functools.lru_cache(None)
def coarse_suite(B, N):
    """near and far distinct per ray (near = 0 on some, > 0 on the others), every kind of direction over the five
    shapes, radii 1e-3 .. 1e-1, t_rand with exact 0 and 1 - eps32."""
    k = COARSE_SHAPES.index((B, N))
    g = torch.Generator().manual_seed(100 + k)
    i = torch.arange(B)
    d = _direction_pool(g)[(i + k) % 8]
    o = torch.randn(B, 3, generator=g) * 2
    r = 10 ** (-3 + 2 * torch.rand(B, generator=g))
    pos = ((i + k) % 2 == 1)
    near = torch.where(pos, 0.5 + 0.37 * i.float(), torch.zeros(B))
    far = near + 2.0 + 1.3 * i.float()
    S = N + 1
    t_rand = torch.rand(B, S, generator=g)
    t_rand[0, 0], t_rand[0, -1] = 0.0, ONE_M
    if B > 1:
        t_rand[-1, S // 2], t_rand[-1, 0] = 0.0, ONE_M
    return dict(o=o, d=d, r=r, near=near, far=far, t_rand=t_rand, pos=pos)


ENV_SHAPES = [(3, 7, 5), (2, 10, 10), (1, 1, 1)]


@functools.lru_cache(None)
def env_suite(B, Dn, Ne):
    """env_near, env_far and env_radii distinct per direction (fp16 values, as the callers up-cast them), D != Ne in
    the first shape, distance with an exact 0, one shared env_rand row with 0 and 1 - eps32."""
    k = ENV_SHAPES.index((B, Dn, Ne))
    g = torch.Generator().manual_seed(200 + k)
    o = torch.randn(B, 3, generator=g) * 2
    d = _unit(g, B)
    dist = torch.rand(B, generator=g) * 4 + 0.5
    dist[0] = 0.0
    j = torch.arange(Dn).float()
    h = lambda a: a.half().float()
    env_rand = torch.rand(Ne + 1, generator=g)
    env_rand[0], env_rand[-1] = 0.0, ONE_M
    return dict(o=o, d=d, dist=dist, env_dirs=h(_unit(g, Dn)), env_radii=h(10 ** (-3 + 2 * torch.rand(Dn, generator=g))),
                env_near=h(0.02 * j), env_far=h(3.0 + 0.5 * j), env_rand=env_rand)


RESAMPLE_N = [2, 3, 63, 64, 65, 129, 449, 511, 512]
RESAMPLE_B = 5  # two blocks of four waves, waves 1 to 3 of the second exit at once
PADDINGS = (0.01, 0.0)


@functools.lru_cache(None)
def resample_suite(N):
    """t_in sorted from 0, ten weight patterns [5, N], one u_rand in [0, 1/S - eps32), rays for the cone."""
    g = torch.Generator().manual_seed(300 + N)
    B, S = RESAMPLE_B, N + 1
    t = torch.sort(torch.rand(B, S, generator=g) * 10, -1).values
    t[:, 0] = 0
    pats = {"rand": torch.rand(B, N, generator=g)}
    sp = torch.zeros(B, N)
    sp[torch.arange(B), torch.tensor([0, N - 1, N // 2, 1 % N, (N - 2) % N])] = 1.0
    pats["spike"] = sp
    pats["big"] = torch.rand(B, N, generator=g) * 50
    pats["tiny"] = torch.rand(B, N, generator=g) * 1e-9
    pats["zeros"] = torch.zeros(B, N)
    pl = torch.zeros(B, N)
    pl[:, N // 3:2 * N // 3 + 1] = 0.25
    pats["plateau"] = pl
    lz = torch.rand(B, N, generator=g)
    lz[:, :N // 2] = 0
    pats["leadzero"] = lz
    tz = torch.rand(B, N, generator=g)
    tz[:, N // 2 + 1:] = 0
    pats["trailzero"] = tz
    pats["ones"] = torch.ones(B, N)
    pats["wide"] = torch.exp(torch.randn(B, N, generator=g) * 4)
    u_rand = torch.rand(B, S, generator=g) * (1.0 / S - EPS32)
    d = _direction_pool(g)[[0, 1, 5, 2, 7]]
    return dict(t=t, pats=pats, u_rand=u_rand, o=torch.randn(B, 3, generator=g) * 2, d=d,
                r=10 ** (-3 + 2 * torch.rand(B, generator=g)))


def resample_cases(N, B=RESAMPLE_B):
    """(label, bins, weights, padding, u_rand or None) of every case of one N, on the first B rays of the suite."""
    s = resample_suite(N)
    for name, w in s["pats"].items():
        for padding in PADDINGS:
            for ur in (None, s["u_rand"]):
                yield (f"N{N}/{name}/pad{padding}/{'rnd' if ur is not None else 'det'}", s["t"][:B].contiguous(),
                       w[:B].contiguous(), padding, None if ur is None else ur[:B].contiguous())


THRESHOLD_MASSES = (8e-6, 2e-5)  # below and above the den < 1e-5 rule
THRESHOLD_SAMPLE = 4             # the sample that u_rand moves onto the small bin's midpoint


@functools.lru_cache(None)
def threshold_case():
    """N = 8, padding 0, weights 1 1 1 e e e 1 1: the blurred bins are 1 1 1 (1+e)/2 e (1+e)/2 1 1, so bin 4 has mass
    e / (6 + 2 e) - 8e-6 on ray 0 (snaps to den = 1: t = b0 + 4e-6 bw) and 2e-5 on ray 1 (ordinary: t = b0 + bw / 2).
    u_rand puts sample 4 on that bin's midpoint and leaves the others at s / S."""
    N, S = 8, 9
    w = torch.ones(2, N)
    u_rand = torch.zeros(2, S)
    for b, m in enumerate(THRESHOLD_MASSES):
        e = 6 * m / (1 - 2 * m)
        w[b, 3:6] = e
        c4 = (3 + 0.5 * (1 + e)) / (6 + 2 * e)
        u_rand[b, THRESHOLD_SAMPLE] = c4 + 0.5 * m - THRESHOLD_SAMPLE * float(f32(1.0 / S))
    t = torch.tensor([0.0, 0.7, 1.9, 3.1, 4.0, 6.5, 7.2, 8.8, 10.0]).repeat(2, 1)
    g = torch.Generator().manual_seed(77)
    return dict(t=t, w=w, u_rand=u_rand, o=torch.randn(2, 3, generator=g), d=_unit(g, 2), r=torch.tensor([0.01, 0.05]))


IPE_M = [1, 5, 341]  # 341 x 48 threads is not a multiple of 256
IPE_COVS = ("zero", "tiny", "typical")


@functools.lru_cache(None)
def ipe_suite(M):
    """means in [-12, 12] with exact zeros, +-10 and fl32(pi); covariances zero (disable_integration: all sixteen
    levels at full amplitude), 1e-12 .. 1e-6 and 1e-6 .. 1."""
    g = torch.Generator().manual_seed(400 + M)
    mean = (torch.rand(M, 3, generator=g) * 2 - 1) * 12
    pi32 = float(f32(np.pi))
    mean[0] = torch.tensor([0.0, -10.0, pi32])
    if M > 2:
        mean[1] = 0.0
        mean[2] = torch.tensor([10.0, pi32, -10.0])
    covs = {"zero": torch.zeros(M, 3), "tiny": 10 ** (-12 + 6 * torch.rand(M, 3, generator=g)),
            "typical": 10 ** (-6 + 6 * torch.rand(M, 3, generator=g))}
    return mean, covs


VIEW_R = [1, 19]  # 19 x 27 = 513 threads


@functools.lru_cache(None)
def view_suite(R):
    g = torch.Generator().manual_seed(500 + R)
    x = _unit(g, R)
    if R >= 6:
        x[1] = torch.tensor([1., 0., 0.])
        x[2] = torch.tensor([0., 0., -1.])
        x[3] = 0.0
        x[4] = _unit(g, 1)[0] * 3.0
        x[5] = torch.tensor([0., -1., 0.])
    return x


LIT_D = [2, 3, 100, 257]
LIT_ARGS = (0.0123456789, 0.1, 7.3)  # radius (not a half value), near, far


# ------------------------------------------------------------------------------------------------- the oracle's own error
@functools.lru_cache(None)
def oracle_t_units():
    """worst error of the fp32 oracle's coarse / env t against fp64, in units, on the suites above: the kernels are
    allowed 4 x these figures and never less than T_FLOOR_UNITS."""
    worst = {"coarse_det": 0.0, "coarse_rnd": 0.0, "coarse_disparity": 0.0, "env_det": 0.0, "env_rnd": 0.0}
    for B, N in COARSE_SHAPES:
        s = coarse_suite(B, N)
        for key, rnd in (("coarse_det", None), ("coarse_rnd", s["t_rand"])):
            got, _ = orc.sample_along_rays(s["o"], s["d"], s["r"].view(-1, 1), N, s["near"].view(-1, 1), s["far"].view(-1, 1), rnd)
            ref, unit = coarse_t64(s["near"], s["far"], N, rnd)
            worst[key] = max(worst[key], units(got, ref, unit))
        p = s["pos"]
        if p.any():
            for rnd in (None, s["t_rand"][p]):
                got, _ = orc.sample_along_rays(s["o"][p], s["d"][p], s["r"][p].view(-1, 1), N, s["near"][p].view(-1, 1),
                                               s["far"][p].view(-1, 1), rnd, disparity=True)
                ref, unit = coarse_t64(s["near"][p], s["far"][p], N, rnd, disparity=True)
                worst["coarse_disparity"] = max(worst["coarse_disparity"], units(got, ref, unit))
    for B, Dn, Ne in ENV_SHAPES:
        s = env_suite(B, Dn, Ne)
        xs = surface_points32(s["o"], s["d"], s["dist"])
        for key, rnd in (("env_det", None), ("env_rnd", s["env_rand"].view(1, -1))):
            got, _, _ = orc.sample_each_points(xs, s["env_dirs"], Ne, s["env_near"].view(-1, 1), s["env_far"].view(-1, 1),
                                               s["env_radii"].view(-1, 1), rnd)
            _, _, _, nr, fr = env_expand(xs, s["env_dirs"], s["env_radii"], s["env_near"], s["env_far"])
            ref, unit = coarse_t64(nr, fr, Ne, rnd)
            worst[key] = max(worst[key], units(got.expand(B * Dn, Ne + 1), ref, unit))
    return worst


def t_bound(key):
    return max(T_FLOOR_UNITS, 4.0 * oracle_t_units()[key])
