"""The exact-fp32 GEMM / MLP family (pn_gemm.hip, pn_mlp.hip) stage by stage against fp64, at C-ABI level.

Every launch of pn_mlp_forward / pn_density_grad / pn_mlp_backward is recomputed in fp64 (torch on the device: rocBLAS fp64 shares
no code with the kernels) from the buffers that launch reads, as the device left them, and compared per element in conditioning
units; tests/_mlp_ref.py states the stages, the units and the bounds, tests/test_mlp_ref_cpu.py checks that restatement on the CPU.
Every buffer an entry point writes is prefilled with NaN (mask words with all-ones bits, `grads` with a non-zero pattern) and has
guard rows behind it.  pn_gemm_nt / pn_gemm_tn are driven directly over tile edges, K tails, leading dimensions wider than the
rows and every flag set the ABI passes.  Run with -s for the worst error of every stage kind and case."""
import ctypes

import pytest
import torch

import _mlp_ref as R
from conftest import gates_of, report_worst

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
GUARD = 8
PN_ERR_BAD_SHAPE, PN_ERR_UNSUPPORTED, PN_ERR_NULL = -1, -2, -3


def dev():
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def lib():
    from pano_nerf_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def e32():
    return R.e32_table()


@pytest.fixture(scope="module")
def weights(lib):
    """{nc: (parameters on the device by name, flat block, packed weights)}"""
    out = {}
    for nc in (5, 1):
        p = R.params(nc)
        flat = R.flat_of(p, nc).to(dev())
        assert int(lib.load().pn_param_layout(nc, None)) == flat.numel()
        wpack = torch.empty(int(lib.load().pn_wpack_floats(nc)), device=dev())
        lib.call("pn_pack_weights", flat.data_ptr(), nc, wpack.data_ptr(), st())
        out[nc] = ({k: v.to(dev()) for k, v in p.items()}, flat, wpack)
    return out


def filled(rows, cols, value=NAN, dtype=torch.float32):
    """[rows + GUARD, cols] filled with `value`: the buffer and its guard rows."""
    return torch.full((rows + GUARD, cols), value, dtype=dtype, device=dev())


def untouched(t, value=NAN):
    return bool(torch.isnan(t).all()) if value != value else bool((t == value).all())


class Eval:
    """one MLP evaluation on the device: its padded buffers (NaN-prefilled, guarded) and the views of rows < M that the reference reads."""

    def __init__(self, lib, case, weights, sparse=False):
        self.lib, self.case = lib, case
        self.inp = R.to_device(R.case_inputs(case, sparse), dev())
        M, V, nc = self.inp["M"], self.inp["V"], self.inp["nc"]
        self.M, self.Mp = M, int(lib.load().pn_pad_rows(M))
        self.p, self.flat, self.wpack = weights[nc]
        Mp = self.Mp
        self.raw = dict(enc=filled(Mp, 96), viewenc=filled(V, 27), viewbias=filled(V, 128), acts=filled(10 * Mp, 256),
                        masks=filled(9 * Mp, 8, -1, torch.int32), raw_rgb=filled(M, 3), raw_density=filled(M, nc),
                        rsweep=filled(8 * Mp, 256), scratch=filled(Mp, 96), grad_mean=filled(M, 3), d_mean=filled(M, 3))
        self.work = None

    def ptr(self, k):
        return self.raw[k].data_ptr()

    def forward(self):
        i = self.inp
        self.lib.call("pn_mlp_forward", self.M, i["rpr"], i["V"], i["nc"], self.flat.data_ptr(), self.wpack.data_ptr(),
                      i["mean"].data_ptr(), i["cov"].data_ptr(), i["vd"].data_ptr(), self.ptr("enc"), self.ptr("viewenc"),
                      self.ptr("viewbias"), self.ptr("acts"), self.ptr("masks"), self.ptr("raw_rgb"), self.ptr("raw_density"), st())

    def density_grad(self):
        i = self.inp
        self.lib.call("pn_density_grad", self.M, i["nc"], i["dbias"], self.flat.data_ptr(), self.wpack.data_ptr(),
                      i["mean"].data_ptr(), i["cov"].data_ptr(), self.ptr("acts"), self.ptr("masks"), self.ptr("raw_density"),
                      self.ptr("rsweep"), self.ptr("scratch"), self.ptr("grad_mean"), st())

    def backward(self, grads, defer=0, deferred=(), v="own", expect=0, **override):
        """pn_mlp_backward with the argument plumbing of render.py::_layer_backward.  deferred: [(Eval, had_tangent)]."""
        i = self.inp
        v = i["v"] if isinstance(v, str) else v
        a = dict(M=self.M, rpr=i["rpr"], V=i["V"], nc=i["nc"], rsweep=self.ptr("rsweep"), n_deferred=len(deferred))
        a.update(override)
        m_batched = self.M * (2 if v is not None else 1) + sum(e.M * (2 if t else 1) for e, t in deferred)
        n = int(self.lib.load().pn_mlp_backward_work_floats(self.M, i["rpr"], i["V"], m_batched if deferred else 0))
        self.work = torch.full((n + GUARD * 256,), NAN, device=dev())
        nd = max(len(deferred), 1)
        dM = (ctypes.c_int64 * nd)(*[e.M for e, _ in deferred])
        denc = (ctypes.c_void_p * nd)(*[e.ptr("enc") for e, _ in deferred])
        dacts = (ctypes.c_void_p * nd)(*[e.ptr("acts") for e, _ in deferred])
        drs = (ctypes.c_void_p * nd)(*[(e.ptr("rsweep") if t else None) for e, t in deferred])
        dwork = (ctypes.c_void_p * nd)(*[e.work.data_ptr() for e, _ in deferred])
        dtan = (ctypes.c_int * nd)(*[int(bool(t)) for _, t in deferred])
        rc = self.lib.load().pn_mlp_backward(
            a["M"], a["rpr"], a["V"], a["nc"], i["dbias"], self.flat.data_ptr(), self.wpack.data_ptr(), i["mean"].data_ptr(),
            i["cov"].data_ptr(), self.ptr("enc"), self.ptr("viewenc"), self.ptr("acts"), self.ptr("masks"), self.ptr("raw_density"),
            i["d_rgb"].data_ptr(), i["d_den"].data_ptr(), a["rsweep"], None if v is None else v.data_ptr(), self.ptr("d_mean"),
            grads.data_ptr(), self.work.data_ptr(), m_batched if deferred else 0, defer, a["n_deferred"], dM, denc, dacts, drs,
            dwork, dtan, st(), None)
        assert rc == expect, (rc, expect)

    def bufs(self, grads=None):
        """views of the rows < M (the kept head of `work` is delta [9], hdot [8], d_bott, edot: carve_keep in pn_mlp.hip)."""
        M, Mp, r = self.M, self.Mp, self.raw
        b = dict(enc=r["enc"][:M], viewenc=r["viewenc"][:-GUARD], viewbias=r["viewbias"][:-GUARD],
                 acts=r["acts"][:10 * Mp].view(10, Mp, 256)[:, :M], masks=r["masks"][:9 * Mp].view(9, Mp, 8)[:, :M],
                 raw_rgb=r["raw_rgb"][:M], raw_density=r["raw_density"][:M], rsweep=r["rsweep"][:8 * Mp].view(8, Mp, 256)[:, :M],
                 scratch=r["scratch"][:M], grad_mean=r["grad_mean"][:M], d_mean=r["d_mean"][:M], grads=grads)
        if self.work is not None:
            w, o = self.work, 0
            for k, planes, cols in (("delta", 9, 256), ("tang", 8, 256), ("d_bott", 1, 256), ("edot", 1, 96)):
                b[k] = w[o:o + planes * Mp * cols].view(planes, Mp, cols)[:, :M]
                o += planes * Mp * cols
            b["d_bott"], b["edot"] = b["d_bott"][0], b["edot"][0]
        return b

    def assert_guards(self):
        M, Mp, r = self.M, self.Mp, self.raw
        for k, t in r.items():
            if k == "masks":
                assert bool((t[-GUARD:] == -1).all()), "guard rows of the mask words were written"
            else:
                assert untouched(t[-GUARD:]), f"guard rows of {k} were written"
        assert untouched(r["acts"][9 * Mp:10 * Mp, 128:]), "columns 128..255 of the view-hidden plane were written"
        assert bool((r["masks"][8 * Mp:9 * Mp, 4:] == -1).all()), "words 4..7 of mask slot 8 were written"
        if self.work is not None:
            assert untouched(self.work[-GUARD * 256:]), "the floats behind the backward workspace were written"


def report(ck, label):
    w = ck.worst()
    print(f"\n{label}: worst units (bound) per stage kind: " + ", ".join(f"{k} {u:.2f} ({b:.0f})" for k, (u, b) in sorted(w.items())))
    for k, (u, b) in w.items():
        report_worst(f"mlp_stages/{k} [units]", u)


def run_case(lib, case, weights, e32, sparse=False):
    ev = Eval(lib, case, weights, sparse)
    pre = R.pattern(ev.flat.numel()).to(dev())
    grads = pre.clone()
    ev.forward()
    ev.density_grad()
    ev.backward(grads)
    torch.cuda.synchronize()
    bufs = ev.bufs(grads)
    ck, _ = R.check(ev.inp, bufs, e32, str(case), prefill=pre, p=ev.p)
    report(ck, str(case))
    return ev, bufs, ck


def assert_case(ev, bufs, ck):
    assert not ck.failures(), ck.failures()   # every checked output within its bound, finite, and zero where its gate bit is clear
    assert R.mask_mismatches(bufs) == [0] * 9, "mask bits differ from (stored activation > 0)"

    class _Ev:
        M, masks = ev.M, bufs["masks"]
    assert bool((gates_of(_Ev, False) == R.unpack_masks(bufs["masks"]).cpu()).all())
    if ev.M >= 65:
        sh = R.gate_shares(bufs)
        assert all(0.05 <= s <= 0.95 for s in sh), sh
    ev.assert_guards()


@pytest.mark.parametrize("case", R.CASES, ids=[str(c[0]) for c in R.CASES])
def test_mlp_stages(lib, weights, e32, case):
    assert_case(*run_case(lib, case, weights, e32))


def test_mlp_stages_large(lib, weights, e32):
    """33000 rows, dense forward, backward seeded in ten rows: k_head_bwd_weight over 258 row blocks, the nine column-sum slots
    over 516 partial rows (two-stage pn_launch_reduce_rows), the view-row fold over 825 partials.  A dropped or doubled block is a
    tenth of a gradient that is a sum over ten rows."""
    ev, bufs, ck = run_case(lib, R.LARGE, weights, e32, sparse=True)
    assert_case(ev, bufs, ck)
    others = torch.tensor([1, 126, 129, 5000, 16382, 16385, 20000, 32766, 32769, 32894, 32897, 32998], device=dev())
    for k in ("delta", "tang"):
        assert bool((bufs[k][:, others] == 0).all()), f"{k} is not zero in rows without an upstream gradient"
    assert bool((bufs["d_bott"][others] == 0).all())


def test_deferred_weight_gradients(lib, weights, e32):
    """evaluations A (65 rows, with v) and E (96 rows) defer their trunk weight gradients, B (129 rows) reduces all three: four
    row segments of 129, 65, 65 and 96 rows in one TN launch per layer, two of them with one-row tails."""
    cA, cE, cB = R.DEFERRED
    A, E, B = Eval(lib, cA, weights), Eval(lib, cE, weights), Eval(lib, cB, weights)
    pre = R.pattern(A.flat.numel()).to(dev())
    grads = pre.clone()
    for ev in (A, E, B):
        ev.forward()
        ev.density_grad()
    A.backward(grads, defer=1)
    E.backward(grads, defer=1)
    B.backward(grads, deferred=[(A, True), (E, False)])
    torch.cuda.synchronize()
    terms, cks = [], []
    for ev in (B, A, E):   # every evaluation's own stages, and its gradient terms from its own buffers
        bufs = ev.bufs(grads)
        ck, hid = R.check(ev.inp, bufs, e32, str(ev.case), p=ev.p)
        assert not ck.failures(), ck.failures()
        terms.append(R.grad_terms(ev.inp, ev.p, bufs, hid))
        ev.assert_guards()
    ck = R.Checker(e32, "deferred")
    for stg in R.grad_stages(terms, 5, grads, pre):
        ck(stg)
    report(ck, "deferred A + E + B")
    assert not ck.failures(), ck.failures()
    # B with a v of its own: own first-order and tangent rows + A's two + E's one = five segments
    vB = R.case_inputs((129, 3, 1, 5, True))["v"].to(dev())
    B.backward(pre.clone(), deferred=[(A, True), (E, False)], v=vB, expect=PN_ERR_UNSUPPORTED)
    torch.cuda.synchronize()


def test_backward_refusals(lib, weights):
    ev = Eval(lib, (65, 5, 13, 5, True), weights)
    ev.forward()
    ev.density_grad()
    pre = R.pattern(ev.flat.numel()).to(dev())
    grads = pre.clone()
    ev.backward(grads, expect=PN_ERR_BAD_SHAPE, rpr=4)           # M % rows_per_ray != 0
    ev.backward(grads, expect=PN_ERR_BAD_SHAPE, V=4)             # (M / rows_per_ray) % view_rows != 0
    ev.backward(grads, expect=PN_ERR_UNSUPPORTED, nc=3)
    ev.backward(grads, expect=PN_ERR_NULL, rsweep=None)          # v without rsweep
    ev.backward(grads, expect=PN_ERR_BAD_SHAPE, n_deferred=3)
    ev.backward(grads, expect=PN_ERR_BAD_SHAPE, defer=1, n_deferred=1)
    torch.cuda.synchronize()
    assert torch.equal(grads, pre) and untouched(ev.work) and untouched(ev.raw["d_mean"]), "a refused call launched work"


# ------------------------------------------------------------------------------------------------- direct GEMM ABI
def _check_direct(stg, got, e32, worst):
    stg.segs = [(a.to(dev()), b.to(dev())) for a, b in stg.segs]
    stg.add = [x.to(dev()) for x in stg.add]
    stg.gate = None if stg.gate is None else stg.gate.to(dev())
    r = R.units(got, R.eval_stage(stg, R.F64), R.unit_of(stg), stg.gate)
    B = R.bound_of(stg, e32)
    worst[0] = max(worst[0], float(r.max()))
    assert int((r > B).sum()) == 0, (stg.name, "units", float(r.max()), "bound", B)


@pytest.mark.parametrize("M", R.NT_M)
def test_gemm_nt_direct(lib, e32, M):
    """lda, ldb, ldc, ldg wider than the rows, sentinel columns behind ldc, NaN in the allocation rows of A beyond M and in its pad
    columns, Inf in those of Bt.  K % 16 != 0 takes k_gemm_nt (20 and 36: its K tail), the others k_gemm_nt_dma (16: one chunk)."""
    worst = [0.0]
    for (m, N, K, flags) in R.nt_combos():
        if m != M:
            continue
        A, Bt, bias, gate, stg = R.nt_case(M, N, K, flags)
        lda, ldb, ldc, ldg = K + 4, K + 8, N + 4, N + 12
        dA, dB = torch.full((M + 3, lda), NAN, device=dev()), torch.full((N + 3, ldb), INF, device=dev())
        dA[:M, :K], dB[:N, :K] = A.to(dev()), Bt.to(dev())
        dC, dG, dbias = filled(M, ldc, 7.0), torch.full((M, ldg), NAN, device=dev()), bias.to(dev())
        dG[:, :N] = gate.to(dev())
        lib.call("pn_gemm_nt", M, N, K, dA.data_ptr(), lda, dB.data_ptr(), ldb, dC.data_ptr(), ldc,
                 dbias.data_ptr() if flags & 1 else None, dG.data_ptr() if flags & 4 else None, ldg, flags, st())
        torch.cuda.synchronize()
        assert bool((dC[:M, N:] == 7.0).all()) and bool((dC[M:] == 7.0).all()), (M, N, K, flags, "sentinels written")
        _check_direct(stg, dC[:M, :N], e32, worst)
    print(f"\npn_gemm_nt M={M}: worst {worst[0]:.2f} units")
    report_worst("mlp_stages/gemm_nt [units]", worst[0])


@pytest.mark.parametrize("N1,N2", R.TN_N)
def test_gemm_tn_direct(lib, e32, N1, N2):
    """accumulate 0 over a NaN-filled C and 1 over a pattern; ldx, ldy, ldc wider than the rows with sentinels; NaN behind the
    M rows of X and Y; work sized by pn_gemm_tn_work_floats with NaN in it and behind it."""
    worst = [0.0]
    for M in R.TN_M:
        for acc in (0, 1):
            X, Y, C0, stg = R.tn_case(M, N1, N2, acc)
            ldx, ldy, ldc = N1 + 4, N2 + 8, N2 + 4
            dX, dY = torch.full((M + 2, ldx), NAN, device=dev()), torch.full((M + 2, ldy), NAN, device=dev())
            dX[:M, :N1], dY[:M, :N2] = X.to(dev()), Y.to(dev())
            dC = filled(N1, ldc, 7.0)
            dC[:N1, :N2] = C0.to(dev()) if acc else NAN
            nw = int(lib.load().pn_gemm_tn_work_floats(M, N1, N2))
            work = torch.full((nw + 64,), NAN, device=dev())
            lib.call("pn_gemm_tn", M, N1, N2, dX.data_ptr(), ldx, dY.data_ptr(), ldy, dC.data_ptr(), ldc, acc, work.data_ptr(), st())
            torch.cuda.synchronize()
            assert bool((dC[:N1, N2:] == 7.0).all()) and bool((dC[N1:] == 7.0).all()), (M, N1, N2, acc, "sentinels written")
            assert untouched(work[nw:]), (M, N1, N2, "floats behind the work buffer written")
            _check_direct(stg, dC[:N1, :N2], e32, worst)
    print(f"\npn_gemm_tn {N1}x{N2}: worst {worst[0]:.2f} units")
    report_worst("mlp_stages/gemm_tn [units]", worst[0])


def test_gemm_refusals(lib):
    """bad arguments are refused with their status code and nothing is launched."""
    L = lib.load()
    A, Bt, C = torch.ones(64, 64, device=dev()), torch.ones(256, 64, device=dev()), torch.full((64, 256), 7.0, device=dev())
    nt = lambda M, N, K, a, lda, ldb=64: L.pn_gemm_nt(M, N, K, a, lda, Bt.data_ptr(), ldb, C.data_ptr(), 256, None, None, 0, 0, st())
    assert nt(64, 128, 6, A.data_ptr(), 8, 8) == PN_ERR_BAD_SHAPE             # K = 6
    assert nt(64, 128, 16, A.data_ptr(), 18) == PN_ERR_BAD_SHAPE              # lda = K + 2
    assert nt(63, 128, 16, A.data_ptr() + 4, 64) == PN_ERR_BAD_SHAPE          # A offset by one float
    assert nt(64, 130, 16, A.data_ptr(), 64) == PN_ERR_BAD_SHAPE              # N = 130
    work = torch.full((int(L.pn_gemm_tn_work_floats(64, 132, 64)),), NAN, device=dev())
    X = torch.ones(64, 136, device=dev())
    tn = lambda N1, w: L.pn_gemm_tn(64, N1, 64, X.data_ptr(), 136, A.data_ptr(), 64, C.data_ptr(), 256, 0, w, st())
    assert tn(130, work.data_ptr()) == PN_ERR_BAD_SHAPE                       # N1 = 130
    assert tn(128, None) == PN_ERR_NULL                                       # null work
    torch.cuda.synchronize()
    assert bool((C == 7.0).all()) and untouched(work), "a refused call launched work"
