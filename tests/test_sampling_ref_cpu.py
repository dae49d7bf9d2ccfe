"""The fp64 restatements of _sampling_ref.py against the fp32 oracle, and the acceptance criteria of
test_gpu_sampling.py on the reference alone: the oracle's own distance from fp64 in the units the GPU tests use (the
figures behind their bounds; printed with -s and kept in profiles/tests_sampling.txt), the 5 % cap on brackets too wide
to see anything, and that the resampling bracket accepts the fp32 oracle and an fp32 emulation of k_resample's summation
order while it rejects six mutated resamplers."""
import numpy as np
import pytest
import torch

import _sampling_ref as ref
from oracle import pano_oracle as orc

f32 = np.float32


# ------------------------------------------------------------------------------------------------- cone -> Gaussian
def cone_rays():
    """4096 rays of 16 intervals from t = 0, with degenerate and one-ulp-wide intervals, axis-aligned, near-axis,
    fp16-rounded and zero directions, radii 1e-3 .. 1e-1."""
    g = torch.Generator().manual_seed(1)
    B, N = 4096, 16
    t = torch.sort(torch.rand(B, N + 1, generator=g) * 10, -1).values
    t[:, 0] = 0
    t[::3, 5] = t[::3, 4]
    t[1::3, 7] = t[1::3, 6] * (1 + 2 * ref.EPS32)
    d = torch.randn(B, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    d[:100] = torch.tensor([0., 0., 1.])
    d[100:200] = torch.tensor([1e-4, 0., 1.])
    d[200:300] = torch.tensor([0., -1., 0.])
    d[300:400] = d[300:400].half().float()
    d[400:420] = 0
    return t, torch.randn(B, 3, generator=g) * 2, d, 10 ** (-3 + 2 * torch.rand(B, 1, generator=g))


def test_cone_restatement_against_the_oracle():
    t, o, d, r = cone_rays()
    assert ref.zero_intervals(t) == 0
    m32, c32 = orc.cast_rays(t, o, d, r)
    mean, cov, umean, ucov = ref.cast_rays64(t, o, d, r)
    em, ec = ref.units(m32, mean, umean), ref.units(c32, cov, ucov)
    print(f"\nfp32 oracle vs fp64, cone -> Gaussian on 4096 x 16 intervals: mean {em:.2f} units, cov {ec:.2f} units")
    # measured 1.6 and 4.35; the kernels' 8 and 16 keep a margin of 4 only while the oracle stays at a quarter of them
    assert em <= ref.MEAN_UNITS / 4 and ec <= ref.COV_UNITS / 3.5, (em, ec)


def test_coarse_and_env_restatements_against_the_oracle():
    worst = ref.oracle_t_units()
    print("\nfp32 oracle vs fp64, t in units of eps32 max(|lower|, |upper|, |t|):",
          ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= ref.T_FLOOR_UNITS, (k, v)  # the kernels' bound max(4, 4 x this) stays within 16 units
    em = ec = 0.0
    for B, N in ref.COARSE_SHAPES:
        s = ref.coarse_suite(B, N)
        for rnd in (None, s["t_rand"]):
            t32, (m32, c32) = orc.sample_along_rays(s["o"], s["d"], s["r"].view(-1, 1), N, s["near"].view(-1, 1),
                                                    s["far"].view(-1, 1), rnd)
            mean, cov, umean, ucov = ref.cast_rays64(t32, s["o"], s["d"], s["r"])  # the cone on the oracle's own t
            em, ec = max(em, ref.units(m32, mean, umean)), max(ec, ref.units(c32, cov, ucov))
    for B, Dn, Ne in ref.ENV_SHAPES:
        s = ref.env_suite(B, Dn, Ne)
        xs = ref.surface_points32(s["o"], s["d"], s["dist"])
        t32, (m32, c32), _ = orc.sample_each_points(xs, s["env_dirs"], Ne, s["env_near"].view(-1, 1),
                                                    s["env_far"].view(-1, 1), s["env_radii"].view(-1, 1),
                                                    s["env_rand"].view(1, -1))
        o, d, rad, _, _ = ref.env_expand(xs, s["env_dirs"], s["env_radii"], s["env_near"], s["env_far"])
        mean, cov, umean, ucov = ref.cast_rays64(t32, o, d, rad)
        em, ec = max(em, ref.units(m32, mean, umean)), max(ec, ref.units(c32, cov, ucov))
    print(f"fp32 oracle vs fp64, cone on the coarse and env suites: mean {em:.2f} units, cov {ec:.2f} units")
    assert em <= ref.MEAN_UNITS / 4 and ec <= ref.COV_UNITS / 3.5, (em, ec)


def test_suites_hold_no_zero_zero_interval():
    """mu = hw = 0 makes the stable-cone formula 0/0, in fp64 too: no suite may contain t0 = t1 = 0."""
    for B, N in ref.COARSE_SHAPES:
        s = ref.coarse_suite(B, N)
        assert bool((s["near"] == 0).any() or B == 1) and bool((s["far"] > s["near"]).all())
        assert len(set(s["near"].tolist())) > 1 or B == 1
        for rnd in (None, s["t_rand"]):
            assert ref.zero_intervals(ref.coarse_t64(s["near"], s["far"], N, rnd)[0]) == 0
        assert float(s["t_rand"].min()) == 0.0 and float(s["t_rand"].max()) == f32(ref.ONE_M)
    for B, Dn, Ne in ref.ENV_SHAPES:
        s = ref.env_suite(B, Dn, Ne)
        assert float(s["dist"][0]) == 0.0
        for rnd in (None, s["env_rand"].view(1, -1)):
            assert ref.zero_intervals(ref.coarse_t64(s["env_near"], s["env_far"], Ne, rnd)[0]) == 0
    for N in ref.RESAMPLE_N:
        for label, t, w, padding, ur in ref.resample_cases(N):
            assert ref.zero_intervals(orc.piecewise_constant_pdf(t, ref.blur(w) + padding, N + 1, ur)) == 0, label


# ------------------------------------------------------------------------------------------------- resampling
def kernel_order_emulation(t, w, padding, ur):
    """k_resample's arithmetic in fp32 numpy, in its order: a run of ceil(N / 64) bins per lane summed serially, a
    butterfly sum / Hillis-Steele scan over the 64 lanes, then the walk along each run."""
    B, N = w.shape
    S, run, lanes = N + 1, (N + 63) // 64, np.arange(64)
    wl = np.zeros((B, 64 * run), f32)
    wl[:, :N] = (ref.blur(w) + float(f32(padding))).numpy()
    wl = wl.reshape(B, 64, run)
    valid = (np.arange(64 * run) < N).reshape(1, 64, run)

    def lane_sums(a):
        s = np.zeros((B, 64), f32)
        for i in range(run):
            s = s + a[:, :, i]
        return s

    v = lane_sums(wl)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    wsum = v[:, 0]
    pad = np.maximum(f32(0), f32(1e-5) - wsum)
    padn, wsum = pad / f32(N), wsum + pad
    p = np.where(valid, (wl + padn[:, None, None]) / wsum[:, None, None], f32(0)).astype(f32)
    ls = lane_sums(p)
    inc, o = ls.copy(), 1
    while o < 64:
        sh = np.concatenate([np.zeros((B, o), f32), inc[:, :-o]], 1)
        inc = np.where(lanes[None] >= o, inc + sh, inc)
        o *= 2
    acc = inc - ls
    cdf = np.zeros((B, S), f32)
    cdf[:, N] = 1
    for i in range(run):
        acc = acc + p[:, :, i]
        n = lanes * run + i
        sel = n < N - 1
        cdf[:, n[sel] + 1] = np.minimum(f32(1), acc[:, sel])
    assert acc.dtype == np.float32 and cdf.dtype == np.float32
    return ref.inverse_cdf(torch.from_numpy(cdf), t, ref.u32(B, S, ur))


MUTATIONS = ("left", "blur1", "nopadn", "shift", "thr", "ustep")


def mutated_resampler(t, w, padding, ur, mut, thr=1e-6):
    """the fp32 oracle with one defect: searchsorted from the left, blur over one neighbour only, pad / N dropped, the
    CDF shifted by one bin, the den threshold at `thr`, a stride of 1 / N for 1 / S in u."""
    B, N = w.shape
    S = N + 1
    if mut == "blur1":
        wp = torch.cat([w[:, :1], w, w[:, -1:]], -1)
        bl = 0.5 * (torch.maximum(wp[:, :-2], wp[:, 1:-1]) + wp[:, 1:-1])
    else:
        bl = ref.blur(w)
    ww = bl + padding
    ws = ww.sum(-1, keepdim=True)
    pad = torch.clamp(1e-5 - ws, min=0)
    if mut != "nopadn":
        ww = ww + pad / N
    pdf = ww / (ws + pad)
    cs = torch.cumsum(pdf[:, 1:] if mut == "shift" else pdf[:, :-1], -1)
    z = torch.zeros(B, 1)
    cdf = torch.cat([z, torch.clamp(cs, max=1.0), z + 1], -1)
    u = ref.u32(B, S, ur)
    if mut == "ustep" and ur is not None:
        u = ((torch.arange(S) * (1 / N))[None] + ur).clamp(max=ref.ONE_M).contiguous()
    idx = torch.searchsorted(cdf, u, right=(mut != "left"))
    lo, hi = (idx - 1).clamp(min=0), idx.clamp(max=S - 1)
    c0, c1 = cdf.gather(-1, lo), cdf.gather(-1, hi)
    b0, b1 = t.gather(-1, lo), t.gather(-1, hi)
    den = c1 - c0
    den = torch.where(den < (thr if mut == "thr" else 1e-5), torch.ones_like(den), den)
    return b0 + (u - c0) / den * (b1 - b0)


@pytest.fixture(scope="module")
def brackets():
    """every resampling case of the GPU test with its bracket, computed once."""
    out = []
    for N in ref.RESAMPLE_N:
        for label, t, w, padding, ur in ref.resample_cases(N):
            u = ref.u32(t.shape[0], N + 1, ur)
            out.append((label, N, t, w, padding, ur, ref.resample_bracket(t, w, padding, u)))
    return out


def test_resample_suites_keep_the_wide_bracket_cap(brackets):
    """A bracket wider than 1e-4 of the ray checks nothing; at most 5 % of a case's samples may have one (N >= 63)."""
    worst = ("", 0.0)
    for label, N, t, w, padding, ur, (lo, hi, tol) in brackets:
        if N >= 63:
            worst = max(worst, (label, ref.wide_share(lo, hi, t)), key=lambda x: x[1])
            assert ref.wide_share(lo, hi, t) <= ref.WIDE_SHARE_CAP, (label, ref.wide_share(lo, hi, t))
    print(f"\nworst share of brackets wider than 1e-4 of the ray: {100 * worst[1]:.2f} % ({worst[0]})")


def test_bracket_accepts_the_oracle_and_the_kernel_order(brackets):
    n = 0
    for label, N, t, w, padding, ur, (lo, hi, tol) in brackets:
        got = orc.piecewise_constant_pdf(t, ref.blur(w) + padding, N + 1, ur)
        assert ref.bracket_excess(got, lo, hi, tol)[0] == 0, ("oracle", label, ref.bracket_excess(got, lo, hi, tol))
        emu = kernel_order_emulation(t, w, padding, ur)
        assert ref.bracket_excess(emu, lo, hi, tol)[0] == 0, ("emulation", label, ref.bracket_excess(emu, lo, hi, tol))
        assert bool((emu[:, 1:] >= emu[:, :-1]).all()), ("emulation not sorted", label)
        n += got.numel()
    print(f"\n{n} samples in {len(brackets)} cases: fp32 oracle and kernel-order emulation inside every bracket")


def test_bracket_rejects_the_mutations(brackets):
    outside = {m: 0 for m in MUTATIONS}
    for label, N, t, w, padding, ur, (lo, hi, tol) in brackets:
        for m in MUTATIONS:
            outside[m] += ref.bracket_excess(mutated_resampler(t, w, padding, ur, m), lo, hi, tol)[0]
    print("\nsamples outside their bracket per mutation:", outside)
    for m in MUTATIONS:
        if m != "thr":  # one sample at most separates 1e-6 from 1e-5 in random suites: the directed case below does
            assert outside[m] > 0, m


def test_threshold_case_separates_the_two_branches():
    c = ref.threshold_case()
    t, w, ur = c["t"], c["w"], c["u_rand"]
    s = ref.THRESHOLD_SAMPLE
    u = ref.u32(2, 9, ur)
    cdf = ref.cdf64(w, 0.0)
    mass = cdf[:, 5] - cdf[:, 4]
    assert abs(float(mass[0]) - 8e-6) < 1e-9 and abs(float(mass[1]) - 2e-5) < 1e-9
    assert bool(((u[:, s].double() - cdf[:, 4]) / mass - 0.5).abs().max() < 0.05)  # u sits on the small bin's midpoint
    lo, hi, tol = ref.resample_bracket(t, w, 0.0, u)
    bw = float(t[0, 5] - t[0, 4])
    # ray 0 snaps to den = 1 (t = b0 + ~4e-6 bw), ray 1 interpolates (t = b0 + bw / 2): both brackets are narrow
    assert float(hi[0, s]) < float(t[0, 4]) + 1e-5 * bw and abs(float(lo[1, s]) - float(t[1, 4]) - 0.5 * bw) < 0.1 * bw
    got = orc.piecewise_constant_pdf(t, ref.blur(w), 9, ur)
    assert ref.bracket_excess(got, lo, hi, tol)[0] == 0
    low = mutated_resampler(t, w, 0.0, ur, "thr", 1e-6)    # ray 0 takes the ordinary branch
    high = mutated_resampler(t, w, 0.0, ur, "thr", 1e-4)   # ray 1 snaps
    for bad, ray in ((low, 0), (high, 1)):
        out = torch.maximum(lo - bad.double(), bad.double() - hi)
        assert float(out[ray, s]) > tol and ref.bracket_excess(bad, lo, hi, tol)[0] == 1, (ray, out)


# ------------------------------------------------------------------------------------------------- encodings
def test_encoding_restatements_against_the_oracle():
    worst = {}
    for M in ref.IPE_M:
        mean, covs = ref.ipe_suite(M)
        for name in ref.IPE_COVS:
            enc, unit, y2, v2 = ref.ipe64(mean, covs[name])
            got = orc.integrated_pos_enc(mean, covs[name], 0, 16)
            worst[name] = max(worst.get(name, 0.0), ref.units(got, enc, unit))
            worst["max |argument|"] = max(worst.get("max |argument|", 0.0), float(y2.abs().max()))
    for R in ref.VIEW_R:
        x = ref.view_suite(R)
        enc, unit, _ = ref.view_enc64(x)
        got = orc.pos_enc(x, 0, 4)
        assert torch.equal(got[:, :3], x)
        worst["view"] = max(worst.get("view", 0.0), ref.units(got, enc, unit))
    print("\nfp32 oracle vs fp64, encodings in units of eps32 exp(-v / 2) + 2^-126:",
          ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert worst["max |argument|"] > 3.9e5  # level 15 at full amplitude: 12 * 2^15
    for k in ref.IPE_COVS + ("view",):
        assert worst[k] <= 2.0, (k, worst[k])  # measured 1.2: the kernels' floor of 4 units leaves the libm a factor 2


# ------------------------------------------------------------------------------------------------- light rays
def test_lit_rays_restatement_and_rounding_ties():
    ties = 0
    for Dn in ref.LIT_D:
        x = ref.lit_rays64(Dn, *ref.LIT_ARGS)
        bits = ref.lit_rays_oracle_bits(Dn, *ref.LIT_ARGS)
        assert x.shape == bits.shape == (14 * Dn,)
        np.testing.assert_array_equal(x.astype(np.float16).view(np.uint16), bits)
        ties += int(ref.near_half_tie(x).sum())
    assert float(np.float16(ref.LIT_ARGS[0])) != ref.LIT_ARGS[0]  # the radius is not a half value
    assert ref.near_half_tie(np.array([1.0 + 2.0 ** -11, 0.0, 1.0, 1.0 + 2.0 ** -11 + 2.0 ** -30])).tolist() == [True, False, False, False]
    assert ref.half_ulps_apart(np.array([0x3c00, 0x8001], np.uint16), np.array([0x3c01, 0x0001], np.uint16)).tolist() == [1, 2]
    print(f"\nlight-ray elements within 2^-40 of an fp16 rounding tie: {ties}")
    assert ties == 0  # so the kernel has to match the oracle bit for bit at these sizes
