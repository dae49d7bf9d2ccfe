"""fp64 restatement, stage by stage, of the exact-fp32 GEMM / MLP family (pn_gemm.hip, pn_mlp.hip), written from the header
comment of pn_mlp.hip and the comments at its launch sites.

Every launch is a STAGE  out = epi(sum_k a_k b_k + addends)  and is recomputed in fp64 from the buffers that launch reads, as
the code under test left them (previous activation plane, recorded mask words, fp32 parameters): errors do not accumulate
along the chain and a failure names the launch.  Three stage forms:
  nt   out[M, N] = gate * relu?(sum_seg A_seg B_seg^T + addends)        forward layers, sweeps, data gradients, heads
  tn   out[N1, N2] = sum_seg X_seg^T Y_seg + addends                     weight / bias gradients (bias: Y = a column of ones)
  fn   a transcendental stage with its own fp64 function and unit       k_dgrad_seed, k_ipe_backward, k_ipe_tangent

Criterion, per element:  unit = 2^-24 (sum_k |a_k| |b_k| + sum |addend|) + 2^-126,  error in units = |got - ref64| / unit,
  bound B = min(max(16, 4 E32), n) + extra       (n: number of summed terms, the order-agnostic worst case)
  fn stages: unit = 2^-24 sum |terms|, bound = max(4, 4 E32) + extra
E32 (e32_table) is the worst error in the same units of the same stage kind evaluated by torch in fp32 on the CPU.

Hidden inputs (dvh, sdot, dden, coef, denc are not exposed by the entry points; S is folded into the view-layer gradient as a
sum over all rows) are recomputed in fp64 from the last exposed buffers.  A stage that consumes one is the composite sum over
both stages' terms: its unit takes the hidden input's own sum of |terms| where it would take |a_k|, and `extra` adds the hidden
stage's own bound: its term count where that is below 16 (3 colour head, nc density head), the GEMM bound for sdot (256 terms)
and denc (512 terms), 4 more for coef and dden (softplus' / softplus'').  So d_mean carries the bounds of its two stages, the
hidden GEMM and the encoding backward.
softplus'' is formed as s (1 - s) = s - s^2, whose fp32 difference cancels for z towards 20: its sum of |terms| is s + s^2.

Where the operation itself holds an fp32 rounding the restatement keeps it, as _sampling_ref.ipe64 does: y = fl32(mean 2^l),
fl32(y + pi/2), z = fl32(raw_density + density_bias).  `exact=True` drops them (the restatement is then the gradient of the fp64
oracle, which test_mlp_ref_cpu.py checks against autograd)."""
import functools

import numpy as np
import torch

from oracle import pano_oracle as orc
from _sampling_ref import ipe_suite

U24, TINY = 2.0 ** -24, 2.0 ** -126
FLOOR, FN_FLOOR = 16.0, 4.0
F64, F32 = torch.float64, torch.float32

# (M, rows_per_ray, view_rows, nc, second-order v)
CASES = [(1, 1, 1, 5, True), (65, 5, 13, 5, True), (127, 1, 127, 1, False), (129, 3, 1, 5, True), (192, 32, 6, 5, False),
         (255, 5, 17, 1, True), (384, 32, 4, 5, True), (496, 16, 31, 5, True), (4100, 4, 1025, 5, True)]
IPE_CASES = {(65, 5, 13, 5, True): "zero", (255, 5, 17, 1, True): "tiny"}  # means / covariances of _sampling_ref.ipe_suite
LARGE = (33000, 8, 5, 5, True)
LARGE_ROWS = (0, 127, 128, 16383, 16384, 32767, 32768, 32895, 32896, 32999)
# density_bias argument per case.  With the trunk weights x 3 the raw density is -160 +- 70 (-395 on the ipe_suite inputs): under
# the product's -1 softplus' underflows to zero in nine rows of ten and the density sweep, the tangent seed and the second-order
# gradients would be checked on zeros.  These values centre z = raw_density + bias, so that nearly every row is live.
DBIAS, DBIAS_IPE = 230.0, 520.0
DEFERRED = [(65, 5, 13, 5, True), (96, 3, 32, 5, False), (129, 3, 1, 5, False)]  # evaluations A, E (deferred) and B (reduces)

NT_M, NT_N, NT_K = (1, 63, 64, 65, 128, 129, 257), (4, 64, 96, 128, 132, 256), (4, 8, 16, 20, 36, 96, 352)
NT_FLAGS = (0, 1, 3, 4, 7)  # BIAS = 1, RELU = 2, GATE = 4
TN_N = ((4, 4), (128, 32), (256, 96), (132, 260), (128, 256), (256, 256))
TN_M = (1, 15, 16, 17, 31, 33, 496, 4100)


def nt_combos():
    """a cross-section of NT_M x NT_N x NT_K x NT_FLAGS: every value of every axis at least five times, every (M, K) pair
    that decides the kernel and its tails, 49 launches."""
    out = []
    for i, M in enumerate(NT_M):
        for j, K in enumerate(NT_K):
            out.append((M, NT_N[(i + 2 * j) % 6], K, NT_FLAGS[(i + j) % 5]))
    return out


# ------------------------------------------------------------------------------------------------- parameters, inputs
ORDER = ([f"layers.{i}.0.{k}" for i in range(8) for k in ("weight", "bias")] +
         ["extra_layer.weight", "extra_layer.bias", "view_layers.0.0.weight", "view_layers.0.0.bias",
          "density_layer.weight", "color_layer.weight", "density_layer.bias", "color_layer.bias"])


@functools.lru_cache(None)
def layout(nc):
    """{name: (offset, shape)} and the total of the flat parameter block (include/panonerf_hip.h)."""
    shapes, off, o = orc.mlp_param_shapes(nc), {}, 0
    for k in ORDER:
        off[k] = (o, tuple(shapes[k]))
        o += int(np.prod(shapes[k]))
    return off, o


@functools.lru_cache(None)
def params(nc):
    """orc.init_params with the trunk weights x 3 (activations spread over several binades, as in test_gpu_chain.py)."""
    p = orc.init_params(21, nc)
    return {k: v * (3.0 if k.endswith("weight") and k.startswith("layers") else 1.0) for k, v in p.items()}


def flat_of(p, nc):
    off, total = layout(nc)
    flat = torch.zeros(total)
    for k, (o, shape) in off.items():
        flat[o:o + p[k].numel()] = p[k].reshape(-1)
    return flat


def pattern(total):
    """the non-zero prefill of `grads`."""
    i = torch.arange(total, dtype=torch.float64)
    return (0.01 * (1 + i % 7) * torch.where(i % 3 == 0, -1.0, 1.0)).float()


@functools.lru_cache(None)
def case_inputs(case, sparse=False):
    M, rpr, V, nc, with_v = case
    g = torch.Generator().manual_seed(1000 + M + (7 if with_v else 0))
    if case in IPE_CASES:
        mean, covs = ipe_suite(M)
        mean, cov = mean.clone(), covs[IPE_CASES[case]].clone()
    else:
        mean = (torch.rand(M, 3, generator=g) - 0.5) * 2
        cov = 1e-3 + torch.rand(M, 3, generator=g) * 1e-2
    vd = torch.nn.functional.normalize(torch.randn(V, 3, generator=g), dim=-1)
    d_rgb, d_den, v = torch.randn(M, 3, generator=g), torch.randn(M, nc, generator=g), torch.randn(M, 3, generator=g)
    if sparse:
        keep = torch.zeros(M, 1)
        keep[list(LARGE_ROWS)] = 1.0
        d_rgb, d_den, v = d_rgb * keep, d_den * keep, v * keep
    return dict(M=M, rpr=rpr, V=V, nc=nc, mean=mean, cov=cov, vd=vd, d_rgb=d_rgb, d_den=d_den, v=v if with_v else None,
                exact=False, dbias=DBIAS_IPE if case in IPE_CASES else DBIAS)


def to_device(inp, device):
    return {k: (x.to(device) if torch.is_tensor(x) else x) for k, x in inp.items()}


def alloc(inp, dt=F32, device="cpu"):
    """the exposed buffers of the three entry points, rows < M only (the tests pass views of the padded device buffers)."""
    M, V, nc = inp["M"], inp["V"], inp["nc"]
    z = lambda *s: torch.zeros(*s, dtype=dt, device=device)
    return dict(enc=z(M, 96), viewenc=z(V, 27), viewbias=z(V, 128), acts=z(10, M, 256),
                masks=torch.zeros(9, M, 8, dtype=torch.int32, device=device), raw_rgb=z(M, 3), raw_density=z(M, nc),
                rsweep=z(8, M, 256), scratch=z(M, 96), grad_mean=z(M, 3), delta=z(9, M, 256), tang=z(8, M, 256),
                d_bott=z(M, 256), edot=z(M, 96), d_mean=z(M, 3), grads=z(layout(nc)[1]))


# ------------------------------------------------------------------------------------------------- mask words
def pack_masks(gate):
    """bool [M, 32 w] -> int32 [M, w]: bit c * 8 + i of word col / 32 <-> column 32 (col / 32) + 4 i + c (pn_common.h)."""
    M, n = gate.shape
    g = gate.view(M, n // 32, 8, 4).to(torch.int64)  # [word, i, c]
    i, c = torch.arange(8, device=gate.device).view(1, 1, 8, 1), torch.arange(4, device=gate.device).view(1, 1, 1, 4)
    w = (g << (c * 8 + i)).sum((2, 3))
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_masks(words, plain=False):
    """int32 [..., w] -> bool [..., 32 w].  plain=True: bit = column & 31, the layout the kernels do NOT use (a mutant)."""
    w = words.to(torch.int64) & 0xffffffff
    col = torch.arange(32 * words.shape[-1], device=words.device)
    bit = (col & 31) if plain else (col & 3) * 8 + ((col & 31) >> 2)
    return ((w[..., col >> 5] >> bit) & 1).bool()


# ------------------------------------------------------------------------------------------------- stages
class Hid:
    """a hidden input: its fp64 value, the sum of |terms| of the stage that made it, that stage's bound in units."""
    def __init__(self, val, absval=None, extra=0.0):
        self.val, self.absval, self.extra = val, absval, extra


def _val(x):
    return x.val if isinstance(x, Hid) else x


def _abs(x):
    return x.absval if isinstance(x, Hid) else x.abs()


def _extra(x):
    return x.extra if isinstance(x, Hid) else 0.0


class Stage:
    def __init__(self, name, kind, form, out=None, segs=(), add=(), relu=False, gate=None, extra=0.0, fn=None, unit=None,
                 mask_out=None, hidden=False, check=True, second=None):
        self.name, self.kind, self.form, self.out, self.segs, self.add = name, kind, form, out, list(segs), list(add)
        self.relu, self.gate, self.extra, self.fn, self.unit, self.mask_out = relu, gate, extra, fn, unit, mask_out
        self.hidden, self.check, self.second = hidden, check, second

    @property
    def terms(self):
        if self.form == "fn":
            return None
        ax = 1 if self.form == "nt" else 0
        return sum(_val(a).shape[ax] for a, _ in self.segs) + len(self.add)

    def mutant(self, **kw):
        """a copy with some fields replaced (the CPU test's wrong evaluations)."""
        st = Stage(self.name, self.kind, self.form)
        st.__dict__.update(self.__dict__)
        st.__dict__.update(kw)
        return st


def eval_stage(st, dt):
    """the stage with every operand cast to dt, products by torch.matmul."""
    if st.form == "fn":
        return st.fn(dt)
    s = 0
    for a, b in st.segs:
        a, b = _val(a).to(dt), _val(b).to(dt)
        s = s + (a @ b.T if st.form == "nt" else a.T @ b)
    for x in st.add:
        s = s + x.to(dt)
    return _epilogue(st, s)


def _epilogue(st, s):
    if st.relu:
        s = torch.relu(s)
    if st.gate is not None:
        s = torch.where(st.gate, s, torch.zeros_like(s))
    return s


def abs_of(st):
    """sum |a_k| |b_k| + sum |addend| per element (a hidden operand enters with its own sum of |terms|)."""
    if st.form == "fn":
        return st.unit()
    u = 0
    for a, b in st.segs:
        a, b = _abs(a).double(), _abs(b).double()
        u = u + (a @ b.T if st.form == "nt" else a.T @ b)
    for x in st.add:
        u = u + x.double().abs()
    if st.gate is not None:
        u = torch.where(st.gate, u, torch.zeros_like(u))
    return u


def unit_of(st):
    return U24 * abs_of(st) + TINY


def stage_extra(st):
    return st.extra + max([0.0] + [max(_extra(a), _extra(b)) for a, b in st.segs])


def bound_of(st, e32):
    e = 4.0 * e32.get(st.kind, 0.0)
    if st.form == "fn":
        return max(FN_FLOOR, e) + stage_extra(st)
    return min(max(FLOOR, e), float(st.terms)) + stage_extra(st)


def units(got, ref, unit, gate=None):
    """|got - ref| / unit per element; exact elements count 0, non-finite ones and non-zero gated ones inf."""
    got = got.double()
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / unit)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    if gate is not None:
        r = torch.where(~gate & (got != 0), torch.full_like(r, float("inf")), r)
    return r


def eval_chain32(st, chunk=32):
    """a second fp32 scheme: per output one sequential chain (separately rounded products and sums) over every `chunk` terms,
    then the partial sums added as a binary tree: the order of a tiled kernel with a split reduction."""
    if st.form == "fn":
        return st.fn(F32)
    parts = []
    for a, b in st.segs:
        a, b = _val(a).float(), _val(b).float()
        if st.form == "tn":
            a, b = a.T, b.T  # [N1, rows], [N2, rows]
        for k0 in range(0, a.shape[1], chunk):
            acc = torch.zeros(a.shape[0], b.shape[0])
            for k in range(k0, min(k0 + chunk, a.shape[1])):
                acc = acc + a[:, k:k + 1] * b[:, k][None, :]
            parts.append(acc)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    s = parts[0]
    for x in st.add:
        s = s + x.float()
    return _epilogue(st, s)


# ------------------------------------------------------------------------------------------------- transcendental pieces
def sp_d1(z):
    return torch.where(z > 20, torch.ones_like(z), 1 / (1 + torch.exp(-z)))


def sp_d2(z):
    s = 1 / (1 + torch.exp(-z))
    return torch.where(z > 20, torch.zeros_like(z), s * (1 - s))


def sp_d2_abs(z):
    """sum of |terms| of softplus'' as the kernels (and torch) form it, s (1 - s) = s - s^2: for z towards 20 the fp32 difference
    1 - s cancels, so the conditioning unit of the product is s + s^2 and not its value."""
    s = 1 / (1 + torch.exp(-z))
    return torch.where(z > 20, torch.zeros_like(z), s * (1 + s))


def z_of(raw_density, dt, exact, dbias):
    """raw_density[:, 0] + density_bias [M, 1]; the fp32 sum is part of the operation."""
    if exact:
        return raw_density[:, :1].to(dt) + dbias
    return (raw_density[:, :1].float() + torch.tensor(dbias, dtype=F32, device=raw_density.device)).to(dt)


def ipe_jac(mean, cov, dt, exact):
    """d enc_f / d mean_c(f) = 2^l exp(-v / 2) cos(y2_f) and the factor 2^l exp(-v / 2) [M, 96]; feature f = half * 48 + 3 l + c."""
    sc = torch.tensor([2.0 ** i for i in range(16)], dtype=F64 if exact else F32, device=mean.device)
    m, c = (mean.double(), cov.double()) if exact else (mean.float(), cov.float())
    y = (m[:, None, :] * sc[:, None]).flatten(-2)
    v = (c[:, None, :] * sc[:, None] ** 2).flatten(-2)
    y2 = torch.cat([y, y + orc.HALF_PI_F32], -1).to(dt)   # fl32(y + pi/2) unless exact
    v2 = torch.cat([v, v], -1).to(dt)
    amp = sc.to(dt).repeat_interleave(3).repeat(2)[None] * torch.exp(-0.5 * v2)
    return amp * torch.cos(y2), amp


def ipe_bwd(denc, mean, cov, dt, exact):
    jac, _ = ipe_jac(mean, cov, dt, exact)
    return (denc.to(dt) * jac).view(-1, 2, 16, 3).sum((1, 2))


def ipe_bwd_unit(absdenc, mean, cov, exact):
    _, amp = ipe_jac(mean, cov, F64, exact)
    return (absdenc.double() * amp).view(-1, 2, 16, 3).sum((1, 2))


def ipe_tan(v, mean, cov, dt, exact):
    jac, _ = ipe_jac(mean, cov, dt, exact)
    return v.to(dt).repeat(1, 32) * jac


# ------------------------------------------------------------------------------------------------- the pipeline
def _P(p, device):
    return {k: x.to(device) for k, x in p.items()}


def pipeline(inp, p, bufs, do, what=("fwd", "dgrad", "bwd"), e32=None):
    """Walks the launches of pn_mlp_forward / pn_density_grad / pn_mlp_backward (without the weight gradients: grad_terms) and
    hands every stage to `do`: Runner writes the stage's value into `bufs`, Checker compares `bufs` with the fp64 value."""
    e32 = e32 or {}
    M, rpr, V, nc, exact = inp["M"], inp["rpr"], inp["V"], inp["nc"], inp["exact"]
    dev = bufs["acts"].device
    W = lambda l: p[f"layers.{l}.0.weight"]
    b = lambda l: p[f"layers.{l}.0.bias"]
    We, be, Wv, bv = p["extra_layer.weight"], p["extra_layer.bias"], p["view_layers.0.0.weight"], p["view_layers.0.0.bias"]
    Wd, bd, Wc, bc = p["density_layer.weight"], p["density_layer.bias"], p["color_layer.weight"], p["color_layer.bias"]
    vrow = (torch.arange(M, device=dev) // rpr) % V
    acts, masks, rs, delta, tang = bufs["acts"], bufs["masks"], bufs["rsweep"], bufs["delta"], bufs["tang"]
    enc, edot, mean, cov = bufs["enc"], bufs["edot"], inp["mean"], inp["cov"]
    hid = {}
    if "fwd" in what:
        # the two encodings are checked per element by test_gpu_sampling.py: here they only feed the simulated device
        do(Stage("enc", "enc", "fn", enc, check=False, fn=lambda dt: _ipe64(mean, cov) if dt == F64 and not exact else
                 orc.integrated_pos_enc(mean.to(dt), cov.to(dt), 0, 16)))
        do(Stage("viewenc", "enc", "fn", bufs["viewenc"], check=False, fn=lambda dt: orc.pos_enc(inp["vd"].to(dt), 0, 4)))
        do(Stage("viewbias", "viewbias", "nt", bufs["viewbias"], [(bufs["viewenc"], Wv[:, 256:])], [bv]))
        for l in range(8):
            segs = [(enc, W(0))] if l == 0 else ([(acts[4], W(5)[:, :256]), (enc, W(5)[:, 256:])] if l == 5 else [(acts[l - 1], W(l))])
            do(Stage(f"h{l}", "nt_layer2" if l == 5 else "nt_layer", "nt", acts[l], segs, [b(l)], relu=True, mask_out=masks[l]))
        do(Stage("raw_density", "head_fwd", "nt", bufs["raw_density"], [(acts[7], Wd)], [bd]))
        do(Stage("bottleneck", "nt_layer", "nt", acts[8], [(acts[7], We)], [be]))
        do(Stage("view_hidden", "nt_view", "nt", acts[9][:, :128], [(acts[8], Wv[:, :256])], [bufs["viewbias"][vrow]], relu=True,
                 mask_out=masks[8][:, :4]))
        do(Stage("raw_rgb", "head_fwd", "nt", bufs["raw_rgb"], [(acts[9][:, :128], Wc)], [bc]))
    G = unpack_masks(masks)  # [9, M, 256]
    if "dgrad" in what:
        z = lambda dt: z_of(bufs["raw_density"], dt, exact, inp["dbias"])
        do(Stage("r7", "seed", "fn", rs[7], gate=G[7],
                 fn=lambda dt: torch.where(G[7], sp_d1(z(dt)) * Wd[:1].to(dt), torch.zeros((), dtype=dt, device=dev)),
                 unit=lambda: torch.where(G[7], (sp_d1(z(F64)) * Wd[:1].double()).abs(), torch.zeros((), dtype=F64, device=dev))))
        for l in range(7, 0, -1):
            do(Stage(f"r{l - 1}", "nt_sweep", "nt", rs[l - 1], [(rs[l], W(l)[:, :256].T)], gate=G[l - 1]))
        do(Stage("dsigma_denc", "nt_denc", "nt", bufs["scratch"], [(rs[0], W(0).T), (rs[5], W(5)[:, 256:].T)]))
        do(Stage("grad_mean", "ipe_bwd", "fn", bufs["grad_mean"], fn=lambda dt: ipe_bwd(bufs["scratch"], mean, cov, dt, exact),
                 unit=lambda: ipe_bwd_unit(bufs["scratch"].abs(), mean, cov, exact)))
    if "bwd" not in what:
        return hid
    v = inp["v"]
    dden = inp["d_den"]
    if v is not None:
        do(Stage("edot", "ipe_tan", "fn", edot, fn=lambda dt: ipe_tan(v, mean, cov, dt, exact),
                 unit=lambda: ipe_tan_unit(v, mean, cov, exact)))
        for l in range(8):
            segs = [(edot, W(0))] if l == 0 else ([(tang[4], W(5)[:, :256]), (edot, W(5)[:, 256:])] if l == 5 else [(tang[l - 1], W(l))])
            do(Stage(f"hdot{l}", "nt_sweep2" if l == 5 else "nt_sweep", "nt", tang[l], segs, gate=G[l]))
        sdot = do(Stage("sdot", "head_fwd", "nt", None, [(tang[7], Wd[:1])], hidden=True))
        z64 = z_of(bufs["raw_density"], F64, exact, inp["dbias"])

        def dden_fn(dt):
            zz = z_of(bufs["raw_density"], dt, exact, inp["dbias"])
            out = inp["d_den"].to(dt).clone()
            out[:, :1] += sp_d2(zz) * _val(sdot).to(dt)
            return out

        def dden_abs():
            out = inp["d_den"].double().abs()
            out[:, :1] += sp_d2_abs(z64) * _abs(sdot)
            return out
        dden = do(Stage("dden", "seed2", "fn", None, fn=dden_fn, unit=dden_abs, hidden=True, extra=_extra(sdot)))
        coef = do(Stage("coef", "seed2", "fn", None, hidden=True, unit=lambda: _pad0(sp_d1(z64), nc),
                        fn=lambda dt: _pad0(sp_d1(z_of(bufs["raw_density"], dt, exact, inp["dbias"])), nc)))
        hid["coef"] = coef
    hid["dden"] = dden
    dvh = do(Stage("dvh", "head_bwd", "nt", None, [(inp["d_rgb"], Wc.T)], gate=G[8][:, :128], hidden=True))
    hid["dvh"] = dvh
    do(Stage("d_bott", "nt_dbott", "nt", bufs["d_bott"], [(dvh, Wv[:, :256].T)]))
    do(Stage("delta8", "head_bwd", "nt", delta[8], [(dden, Wd.T)]))
    do(Stage("delta7", "nt_sweep", "nt", delta[7], [(bufs["d_bott"], We.T)], [delta[8]], gate=G[7]))
    for l in range(7, 0, -1):
        do(Stage(f"delta{l - 1}", "nt_sweep", "nt", delta[l - 1], [(delta[l], W(l)[:, :256].T)], gate=G[l - 1]))
    denc = do(Stage("denc", "nt_denc", "nt", None, [(delta[0], W(0).T), (delta[5], W(5)[:, 256:].T)], hidden=True))
    do(Stage("d_mean", "ipe_bwd", "fn", bufs["d_mean"], fn=lambda dt: ipe_bwd(_val(denc), mean, cov, dt, exact),
             unit=lambda: ipe_bwd_unit(_abs(denc), mean, cov, exact), extra=_extra(denc)))
    return hid


def _pad0(col, nc):
    """[M, 1] -> [M, nc] with the column in front (coef enters row 0 of dWd only)."""
    out = torch.zeros(col.shape[0], nc, dtype=col.dtype, device=col.device)
    out[:, :1] = col
    return out


def _ipe64(mean, cov):
    from _sampling_ref import ipe64
    return ipe64(mean.cpu().float(), cov.cpu().float())[0].to(mean.device)


def ipe_tan_unit(v, mean, cov, exact):
    _, amp = ipe_jac(mean, cov, F64, exact)
    return v.double().abs().repeat(1, 32) * amp


def grad_terms(inp, p, bufs, hid):
    """{parameter name: (kind, [(X, Y), ...])}: the weight and bias gradients of ONE evaluation as sums over its rows,
    dP = sum X^T Y (a bias: Y = ones).  The formulas of pn_mlp.hip's launch sites: dWv[:, 256:] = sum_rows dvh[row]^T viewenc[its
    view row]; dbd / dWd from dden_use, with v also coef * hdot_7 into row 0 of dWd; with v every trunk layer adds r_l^T hdot_{l-1}."""
    M, rpr, V, nc = inp["M"], inp["rpr"], inp["V"], inp["nc"]
    dev = bufs["acts"].device
    acts, rs, delta, tang, enc, edot = bufs["acts"], bufs["rsweep"], bufs["delta"], bufs["tang"], bufs["enc"], bufs["edot"]
    vrow = (torch.arange(M, device=dev) // rpr) % V
    one = torch.ones(M, 1, dtype=acts.dtype, device=dev)
    second = inp["v"] is not None
    dvh, dden = hid["dvh"], hid["dden"]
    T = {"color_layer.weight": ("head_wgrad", [(inp["d_rgb"], acts[9][:, :128])]), "color_layer.bias": ("bias", [(inp["d_rgb"], one)]),
         "density_layer.weight": ("head_wgrad", [(dden, acts[7])] + ([(hid["coef"], tang[7])] if second else [])),
         "density_layer.bias": ("bias", [(dden, one)]),
         "view_layers.0.0.weight": ("view_wgrad", [(dvh, torch.cat([acts[8], bufs["viewenc"][vrow].to(acts.dtype)], 1))]),
         "view_layers.0.0.bias": ("bias", [(dvh, one)]),
         "extra_layer.weight": ("wgrad", [(bufs["d_bott"], acts[7])]), "extra_layer.bias": ("bias", [(bufs["d_bott"], one)])}
    for l in range(8):
        prev = enc if l == 0 else (torch.cat([acts[4], enc], 1) if l == 5 else acts[l - 1])
        segs = [(delta[l], prev)]
        if second:
            segs.append((rs[l], edot if l == 0 else (torch.cat([tang[4], edot], 1) if l == 5 else tang[l - 1])))
        T[f"layers.{l}.0.weight"] = ("wgrad", segs)
        T[f"layers.{l}.0.bias"] = ("bias", [(delta[l], one)])
    return T


def grad_stages(term_dicts, nc, grads, prefill):
    """one tn stage per parameter tensor over the rows of every evaluation in `term_dicts`, on top of the prefill pattern."""
    off, _ = layout(nc)
    out = []
    for k in ORDER:
        o, shape = off[k]
        shape2 = shape if len(shape) == 2 else (shape[0], 1)
        n = shape2[0] * shape2[1]
        segs = [s for T in term_dicts for s in T[k][1]]
        out.append(Stage(k, term_dicts[0][k][0], "tn", grads[o:o + n].view(shape2), segs, [prefill[o:o + n].view(shape2)]))
    return out


class Runner:
    """writes every stage's value, computed by `ev`, into its buffer (a simulated device)."""
    def __init__(self, ev):
        self.ev = ev

    def __call__(self, st):
        val = self.ev(st)
        if st.hidden:
            return Hid(val)
        st.out.copy_(val)
        if st.mask_out is not None:
            st.mask_out.copy_(pack_masks(st.out > 0))


class Checker:
    """compares every stage's buffer with the fp64 value of the stage on the buffers it reads."""
    def __init__(self, e32, label=""):
        self.e32, self.label, self.rows, self.stages = e32, label, [], {}

    def __call__(self, st):
        self.stages[st.name] = st
        if not st.check:
            return None
        ref = eval_stage(st, F64)
        if st.hidden:
            return Hid(ref, abs_of(st), bound_of(st, self.e32))
        B = bound_of(st, self.e32)
        r = units(st.out, ref, unit_of(st), st.gate)
        self.rows.append(dict(case=self.label, name=st.name, kind=st.kind, units=float(r.max()), bound=B, bad=int((r > B).sum()),
                              n=st.terms))
        return None

    def worst(self):
        w = {}
        for r in self.rows:
            a = w.get(r["kind"], (0.0, 0.0))
            w[r["kind"]] = (max(a[0], r["units"]), max(a[1], r["bound"]))
        return w

    def failures(self):
        return [r for r in self.rows if r["bad"]]


def mask_mismatches(bufs):
    """slots 0..7 against acts[0..7] > 0, slot 8 against acts[9][:, :128] > 0: the number of differing bits per slot."""
    G = unpack_masks(bufs["masks"])
    bad = [int((G[l] != (bufs["acts"][l] > 0)).sum()) for l in range(8)]
    return bad + [int((G[8][:, :128] != (bufs["acts"][9][:, :128] > 0)).sum())]


def gate_shares(bufs):
    G = unpack_masks(bufs["masks"])
    return [float(G[l].double().mean()) for l in range(8)] + [float(G[8][:, :128].double().mean())]


def simulate(inp, ev=None, what=("fwd", "dgrad", "bwd"), dt=F32, prefill=None):
    """every exposed buffer of one evaluation on a simulated device: stage by stage with the evaluator `ev` (default torch in dt)."""
    ev = ev or (lambda st: eval_stage(st, dt))
    p = params(inp["nc"])
    bufs = alloc(inp, dt)
    hid = pipeline(inp, p, bufs, Runner(ev), what)
    if "bwd" in what:
        pre = torch.zeros_like(bufs["grads"]) if prefill is None else prefill.to(dt)
        for st in grad_stages([grad_terms(inp, p, bufs, hid)], inp["nc"], bufs["grads"], pre):
            Runner(ev)(st)
    return bufs


def check(inp, bufs, e32, label="", what=("fwd", "dgrad", "bwd"), prefill=None, p=None):
    """-> Checker over every stage of one evaluation (weight gradients included when `prefill` is given)."""
    p = p or params(inp["nc"])
    ck = Checker(e32, label)
    hid = pipeline(inp, p, bufs, ck, what, e32)
    if "bwd" in what and prefill is not None:
        for st in grad_stages([grad_terms(inp, p, bufs, hid)], inp["nc"], bufs["grads"], prefill):
            ck(st)
    return ck, hid


# ------------------------------------------------------------------------------------------------- direct GEMM stages
def nt_case(M, N, K, flags, seed=0):
    """operands of one pn_gemm_nt launch and its stage (bias -> ReLU -> gate, as nt_epi_slab applies them)."""
    g = torch.Generator().manual_seed(seed + 7919 * M + 131 * N + K)
    A, Bt = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias, gate = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    st = Stage(f"nt {M}x{N}x{K} f{flags}", "gemm_nt", "nt", None, [(A, Bt)], [bias] if flags & 1 else [], relu=bool(flags & 2),
               gate=(gate > 0) if flags & 4 else None)
    return A, Bt, bias, gate, st


def tn_case(M, N1, N2, accumulate, seed=0):
    g = torch.Generator().manual_seed(seed + 7919 * M + 131 * N1 + N2)
    X, Y = torch.randn(M, N1, generator=g), torch.randn(M, N2, generator=g)
    C0 = pattern(N1 * N2).view(N1, N2) * 100
    st = Stage(f"tn {M}x{N1}x{N2} a{accumulate}", "gemm_tn", "tn", None, [(X, Y)], [C0] if accumulate else [])
    return X, Y, C0, st


# ------------------------------------------------------------------------------------------------- the fp32 oracle's own error
@functools.lru_cache(None)
def e32_table():
    """{stage kind: worst error in units of torch fp32 on the CPU} over CASES, the deferred evaluations and the direct GEMM
    shapes (the large case has the same stage kinds at the same K; its gradients are sums of ten rows)."""
    worst = {}

    def note(kind, u):
        worst[kind] = max(worst.get(kind, 0.0), u)
    for case in CASES + DEFERRED[1:]:
        inp = case_inputs(case)
        pre = pattern(layout(inp["nc"])[1])
        bufs = simulate(inp, prefill=pre)
        ck, _ = check(inp, bufs, {}, prefill=pre)
        for r in ck.rows:
            note(r["kind"], r["units"])
    for (M, N, K, flags) in nt_combos():
        st = nt_case(M, N, K, flags)[4]
        note("gemm_nt", float(units(eval_stage(st, F32), eval_stage(st, F64), unit_of(st), st.gate).max()))
    for (N1, N2) in TN_N:
        for M in TN_M:
            for acc in (0, 1):
                st = tn_case(M, N1, N2, acc)[3]
                note("gemm_tn", float(units(eval_stage(st, F32), eval_stage(st, F64), unit_of(st)).max()))
    return worst
