"""CPU checks of tests/_mlp_ref.py, the fp64 restatement that test_gpu_mlp_stages.py holds the exact-fp32 GEMM / MLP kernels to:
the chained stages are the true gradient (against autograd of the fp64 oracle), the mask-word layout, the fp32 oracle's own error
per stage kind (E32, the figure the bounds are built from), two fp32 evaluation schemes that the bounds must accept, ten wrong
evaluations that they must reject, and the 5 % .. 95 % gate shares of the chosen parameters.  Run with -s for the figures."""
import pytest
import torch

import _mlp_ref as R
from conftest import gates_of
from oracle import pano_oracle as orc

F32, F64 = torch.float32, torch.float64


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-300))


def _autograd(inp, with_v):
    M, rpr, V, nc = inp["M"], inp["rpr"], inp["V"], inp["nc"]
    p64 = {k: x.double().requires_grad_(True) for k, x in R.params(nc).items()}
    vrow = (torch.arange(M) // rpr) % V
    mean64 = inp["mean"].double().requires_grad_(True)
    enc = orc.integrated_pos_enc(mean64.view(M, 1, 3), inp["cov"].double().view(M, 1, 3), 0, 16)
    rgb, den = orc.mlp_forward(p64, enc, orc.pos_enc(inp["vd"].double()[vrow], 0, 4))
    sigma = torch.nn.functional.softplus(den[..., :1] + inp["dbias"])
    (gm,) = torch.autograd.grad(sigma.sum(), mean64, create_graph=True)
    L = (rgb.view(M, 3) * inp["d_rgb"].double()).sum() + (den.view(M, nc) * inp["d_den"].double()).sum()
    if with_v:
        L = L + (gm * inp["v"].double()).sum()
    g = torch.autograd.grad(L, list(p64.values()) + [mean64])
    return rgb.view(M, 3), den.view(M, nc), gm, dict(zip(p64.keys(), g[:-1])), g[-1]


@pytest.mark.parametrize("nc", [5, 1])
def test_restatement_is_the_gradient(nc):
    """the fp64 stage functions chained with natural gates == autograd of L = <d_rgb, raw_rgb> + <d_den, raw_density> +
    <v, d sigma / d mean> through orc.mlp_forward / orc.integrated_pos_enc, to 1e-10 of every tensor's largest element.
    d_mean is the first-order gradient (include/panonerf_hip.h): it is compared in the run without v."""
    base = R.case_inputs((65, 5, 13, nc, True))
    off, _ = R.layout(nc)
    for with_v in (True, False):
        inp = dict(base, exact=True, v=base["v"] if with_v else None)
        bufs = R.simulate(inp, dt=F64)
        rgb, den, gm, gp, dmean = _autograd(inp, with_v)
        assert _rel(bufs["raw_rgb"], rgb) < 1e-10 and _rel(bufs["raw_density"], den) < 1e-10
        assert _rel(bufs["grad_mean"], gm) < 1e-10
        for k, (o, shape) in off.items():
            got = bufs["grads"][o:o + gp[k].numel()].view(gp[k].shape)
            assert _rel(got, gp[k]) < 1e-10, (k, with_v, _rel(got, gp[k]))
        if not with_v:
            assert _rel(bufs["d_mean"], dmean) < 1e-10


def test_mask_words():
    """pack / unpack round-trip, the layout of pn_common.h bit by bit, and conftest.gates_of(ev, False) on the same words."""
    g = torch.Generator().manual_seed(3)
    gate = torch.rand(9, 37, 256, generator=g) > 0.5
    words = torch.stack([R.pack_masks(gate[s]) for s in range(9)])
    assert words.dtype == torch.int32 and words.shape == (9, 37, 8)
    assert bool((R.unpack_masks(words) == gate).all())
    one = torch.zeros(1, 256, dtype=torch.bool)
    one[0, 32 * 5 + 4 * 6 + 3] = True   # column 32 w + 4 i + c with w = 5, i = 6, c = 3 -> bit c * 8 + i = 30 of word 5
    assert R.pack_masks(one)[0].tolist() == [0, 0, 0, 0, 0, 1 << 30, 0, 0]
    one[0, 32 * 5 + 4 * 6 + 3], one[0, 31] = False, True   # i = 7, c = 3 -> bit 31: the sign bit of an int32 word
    assert R.pack_masks(one)[0].tolist() == [-2 ** 31, 0, 0, 0, 0, 0, 0, 0]

    class Ev:
        M = 37
        masks = words
    assert bool((gates_of(Ev, False) == gate).all())
    assert not bool((R.unpack_masks(words, plain=True) == gate).all())


@pytest.fixture(scope="module")
def sims():
    """torch-fp32 simulated device buffers of every case, their checked stages and the prefill (computed once, left unchanged)."""
    e32 = R.e32_table()
    out = {}
    for case in R.CASES:
        inp = R.case_inputs(case)
        pre = R.pattern(R.layout(inp["nc"])[1])
        bufs = R.simulate(inp, prefill=pre)
        ck, _ = R.check(inp, bufs, e32, str(case), prefill=pre)
        out[case] = (inp, bufs, ck, pre)
    return out


def test_e32_and_torch_fp32_within_bound(sims):
    e32 = R.e32_table()
    print("\nE32 (worst error of torch fp32 on the CPU, in units) per stage kind:")
    for k in sorted(e32):
        print(f"  {k:12s} {e32[k]:6.2f}")
    over = sorted(k for k, v in e32.items() if 4 * v > R.FLOOR and not k.startswith(("seed", "ipe")))
    print("kinds whose bound is 4 x E32 and not the floor of 16 units:", over)
    # a sum whose largest term comes early rounds every later addition at that term's ulp: up to n / 2 units, and the ipe_suite
    # inputs (sixteen octaves at full amplitude) make such sums.  None may reach the point where 4 x E32 stops rejecting a bf16
    # operand (several hundred units)
    assert max(e32.values()) < 25.0, e32
    for case, (_, bufs, ck, _) in sims.items():
        assert not ck.failures(), ck.failures()
        assert R.mask_mismatches(bufs) == [0] * 9


def test_chain_emulation_within_bound():
    """the second fp32 scheme (a sequential chain per 32 terms, the partial sums as a tree) on the cases up to 129 rows."""
    e32 = R.e32_table()
    worst = {}
    for case in R.CASES[:4]:
        inp = R.case_inputs(case)
        pre = R.pattern(R.layout(inp["nc"])[1])
        bufs = R.simulate(inp, ev=R.eval_chain32, prefill=pre)
        ck, _ = R.check(inp, bufs, e32, str(case), prefill=pre)
        assert not ck.failures(), ck.failures()
        for k, (u, b) in ck.worst().items():
            worst[k] = max(worst.get(k, 0.0), u)
    print("\nchain emulation, worst units per kind:", {k: round(v, 2) for k, v in sorted(worst.items())})


def _caught(st, mut_value, e32):
    r = R.units(mut_value, R.eval_stage(st, F64), R.unit_of(st), st.gate)
    return int((r > R.bound_of(st, e32)).sum()), r.numel()


def test_bound_rejects_mutants(sims):
    """ten wrong fp32 evaluations, each at the smallest case where it applies: at least one element beyond the bound."""
    e32 = R.e32_table()
    ev = lambda st: R.eval_stage(st, F32)
    S = lambda case, name: sims[case][2].stages[name]
    c1, c65, c129, c255 = R.CASES[0], R.CASES[1], R.CASES[3], R.CASES[5]
    counts = {}
    st = S(c1, "h1")
    a, b = st.segs[0]
    counts["last four k of a segment dropped"] = _caught(st, ev(st.mutant(segs=[(a[:, :-4], b[:, :-4])])), e32)
    st = S(c1, "h5")
    w5 = R.params(5)["layers.5.0.weight"]
    wrong = w5.reshape(-1)[256:].as_strided((256, 96), (256, 1))
    counts["second K segment read with ld 256"] = _caught(st, ev(st.mutant(segs=[st.segs[0], (st.segs[1][0], wrong)])), e32)
    st = S(c1, "h1")
    counts["one operand rounded to bf16"] = _caught(st, ev(st.mutant(segs=[(a.bfloat16().float(), b)])), e32)
    st = S(c1, "layers.3.0.bias")
    x = st.segs[0][0]
    counts["pad rows add a clamped row M-1 to a column sum"] = _caught(st, ev(st) + 127 * x[-1:].T.float(), e32)
    inp, bufs = sims[c255][0], sims[c255][1]   # the smallest case with more rays than view rows and more than one view row
    st = S(c255, "view_hidden")
    ray = (torch.arange(inp["M"]) // inp["rpr"]).clamp(max=inp["V"] - 1)   # no % view_rows (clamped into the buffer)
    counts["row bias indexed without % view_rows"] = _caught(st, ev(st.mutant(add=[bufs["viewbias"][ray]])), e32)
    st = S(c1, "r6")
    plain = R.unpack_masks(sims[c1][1]["masks"], plain=True)[6]
    counts["mask bits in plain column order"] = _caught(st, ev(st.mutant(gate=plain)), e32)
    st = S(c65, "layers.3.0.weight")
    cut = lambda t: torch.cat([t[:32], t[64:]])
    counts["one 32-row chunk of a TN segment dropped"] = _caught(
        st, ev(st.mutant(segs=[(cut(st.segs[0][0]), cut(st.segs[0][1]))] + st.segs[1:])), e32)
    st = S(c1, "layers.3.0.weight")
    x, y = st.segs[0]
    counts["a segment's tail row added twice"] = _caught(st, ev(st.mutant(segs=st.segs + [(x[-1:], y[-1:])])), e32)
    counts["accumulate ignoring C"] = _caught(st, ev(st.mutant(add=[])), e32)
    st = S(c129, "layers.3.0.weight")   # 129 + 129 rows: the first case whose TN launch has more than one split
    x, y = st.segs[0]
    counts["one split slab dropped from the reduction"] = _caught(st, ev(st.mutant(segs=[(x[:96], y[:96])] + st.segs[1:])), e32)
    print("\nmutants: elements beyond the bound / elements")
    for k, (n, tot) in counts.items():
        print(f"  {k:48s} {n:7d} / {tot}")
    assert len(counts) == 10 and all(n >= 1 for n, _ in counts.values()), counts


def test_gate_shares():
    """every slot of every case with M >= 65, and of the large case, has between 5 % and 95 % of its bits set in the fp64 forward."""
    for case in R.CASES + [R.LARGE] + R.DEFERRED[1:]:
        if case[0] < 65:
            continue
        bufs = R.simulate(R.case_inputs(case), what=("fwd",), dt=F64)
        sh = R.gate_shares(bufs)
        print(case, [round(s, 2) for s in sh])
        assert all(0.05 <= s <= 0.95 for s in sh), (case, sh)
