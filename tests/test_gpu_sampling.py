"""The sampling and encoding kernels of pn_render.hip through the C ABI against the fp64 restatements of
_sampling_ref.py, at the shapes where they can go wrong and per element in conditioning units (see that module; the
bounds are derived there and in test_sampling_ref_cpu.py, the measured figures are in profiles/tests_sampling.txt).

Every output buffer is a few rows longer than the kernel may write and pre-filled with a sentinel: the rows beyond the
logical size must still hold it afterwards, and a logical element the kernel skipped fails its comparison."""
import numpy as np
import pytest
import torch

import _sampling_ref as ref
from conftest import report_worst
from oracle import pano_oracle as orc

pytestmark = pytest.mark.gpu
SENTINEL = -7.0e30
EXTRA = 3


@pytest.fixture(scope="module")
def lib():
    from pano_nerf_amd import _lib
    return _lib


def dev():
    return torch.device("cuda:0")


def G(a):
    return None if a is None else torch.as_tensor(a, dtype=torch.float32).contiguous().to(dev())


def st():
    return torch.cuda.current_stream().cuda_stream


def guarded(rows, cols):
    return torch.full((rows + EXTRA, cols), SENTINEL, dtype=torch.float32, device=dev())


def logical(buf, rows, what):
    torch.cuda.synchronize()
    h = buf.cpu()
    assert bool((h[rows:] == SENTINEL).all()), f"{what}: written beyond row {rows}"
    return h[:rows]


def check_cone(label, t, mean, cov, o, d, r):
    """mean / cov [R, N, 3] of the kernel against the fp64 cone formula on the kernel's own t [R, N + 1]."""
    assert ref.zero_intervals(t) == 0, label
    m64, c64, um, uc = ref.cast_rays64(t, o, d, r)
    em, ec = ref.units(mean, m64, um), ref.units(cov, c64, uc)
    kind = label.split("/")[0]
    report_worst(f"sampling/{kind} mean (units, bound {ref.MEAN_UNITS:g})", em)
    report_worst(f"sampling/{kind} cov (units, bound {ref.COV_UNITS:g})", ec)
    assert em <= ref.MEAN_UNITS, (label, "mean", em)
    assert ec <= ref.COV_UNITS, (label, "cov", ec)


def check_t(label, key, t, t64, unit):
    e, bound = ref.units(t, t64, unit), ref.t_bound(key)
    report_worst(f"sampling/{key} t (units, bound {bound:.2f} = max(4, 4 x oracle {ref.oracle_t_units()[key]:.2f}))", e)
    assert e <= bound, (label, key, e, bound)


# ------------------------------------------------------------------------------------------------- coarse
@pytest.mark.parametrize("B,N", ref.COARSE_SHAPES)
def test_sample_coarse(lib, B, N):
    s = ref.coarse_suite(B, N)
    runs = [("coarse_det", False, None, None), ("coarse_rnd", False, None, s["t_rand"])]
    if bool(s["pos"].any()):  # disparity needs near > 0
        runs += [("coarse_disparity", True, s["pos"], None), ("coarse_disparity", True, s["pos"], s["t_rand"])]
    for key, disparity, sel, rnd in runs:
        pick = (lambda a: a) if sel is None else (lambda a: a[sel].contiguous())
        o, d, r, nr, fr = (pick(s[k]) for k in ("o", "d", "r", "near", "far"))
        rnd = None if rnd is None else pick(rnd)
        n, S = o.shape[0], N + 1
        do, dd, dr, dn, df, drnd = G(o), G(d), G(r), G(nr), G(fr), G(rnd)
        t, m, c = guarded(n, S), guarded(n * N, 3), guarded(n * N, 3)
        lib.call("pn_sample_coarse", n, N, int(disparity), do.data_ptr(), dd.data_ptr(), dr.data_ptr(), dn.data_ptr(),
                 df.data_ptr(), lib.ptr(drnd), t.data_ptr(), m.data_ptr(), c.data_ptr(), st())
        label = f"coarse/{B}x{N}/{key}/{'rnd' if rnd is not None else 'det'}"
        t, m, c = logical(t, n, label), logical(m, n * N, label), logical(c, n * N, label)
        t64, unit = ref.coarse_t64(nr, fr, N, rnd, disparity)
        check_t(label, key, t, t64, unit)
        check_cone(label, t, m.view(n, N, 3), c.view(n, N, 3), o, d, r)


# ------------------------------------------------------------------------------------------------- env
@pytest.mark.parametrize("B,Dn,Ne", ref.ENV_SHAPES)
def test_sample_env(lib, B, Dn, Ne):
    s = ref.env_suite(B, Dn, Ne)
    dv = {k: G(s[k]) for k in ("o", "d", "dist", "env_dirs", "env_radii", "env_near", "env_far")}
    xs = ref.surface_points32(s["o"], s["d"], s["dist"])
    o, d, rad, nr, fr = ref.env_expand(xs, s["env_dirs"], s["env_radii"], s["env_near"], s["env_far"])
    R = B * Dn
    for key, rnd in (("env_det", None), ("env_rnd", s["env_rand"])):
        drnd = G(rnd)
        t, m, c = guarded(R, Ne + 1), guarded(R * Ne, 3), guarded(R * Ne, 3)
        lib.call("pn_sample_env", B, Dn, Ne, dv["o"].data_ptr(), dv["d"].data_ptr(), dv["dist"].data_ptr(),
                 dv["env_dirs"].data_ptr(), dv["env_radii"].data_ptr(), dv["env_near"].data_ptr(), dv["env_far"].data_ptr(),
                 lib.ptr(drnd), t.data_ptr(), m.data_ptr(), c.data_ptr(), st())
        label = f"env/{B}x{Dn}x{Ne}/{key}"
        t, m, c = logical(t, R, label), logical(m, R * Ne, label), logical(c, R * Ne, label)
        t64, unit = ref.coarse_t64(nr, fr, Ne, None if rnd is None else rnd.view(1, -1))
        check_t(label, key, t, t64, unit)  # all B * D rows
        check_cone(label, t, m.view(R, Ne, 3), c.view(R, Ne, 3), o, d, rad)


# ------------------------------------------------------------------------------------------------- resample
def run_resample(lib, t_in, w, padding, ur, o, d, r, label):
    B, N = w.shape
    keep = [G(t_in), G(w), G(ur), G(o), G(d), G(r)]
    t, m, c = guarded(B, N + 1), guarded(B * N, 3), guarded(B * N, 3)
    lib.call("pn_resample", B, N, keep[0].data_ptr(), keep[1].data_ptr(), padding, lib.ptr(keep[2]), keep[3].data_ptr(),
             keep[4].data_ptr(), keep[5].data_ptr(), t.data_ptr(), m.data_ptr(), c.data_ptr(), st())
    return logical(t, B, label), logical(m, B * N, label).view(B, N, 3), logical(c, B * N, label).view(B, N, 3)


def check_bracket(label, t, t_in, w, padding, ur):
    lo, hi, tol = ref.resample_bracket(t_in, w, padding, ref.u32(t.shape[0], t.shape[1], ur))
    bad, worst = ref.bracket_excess(t, lo, hi, tol)
    report_worst("sampling/resample t (distance outside the +-16 eps32 bracket over tol = 4 eps32 max|bins|, bound 1)", worst)
    assert bad == 0, (label, "samples outside their bracket", bad, "worst, in tol", worst)


@pytest.mark.parametrize("N", ref.RESAMPLE_N)
@pytest.mark.parametrize("B", [ref.RESAMPLE_B, 1])
def test_resample(lib, B, N):
    s = ref.resample_suite(N)
    o, d, r = s["o"][:B], s["d"][:B], s["r"][:B]
    for label, t_in, w, padding, ur in ref.resample_cases(N, B):
        label = f"resample/B{B}/{label}"
        t, m, c = run_resample(lib, t_in, w, padding, ur, o, d, r, label)
        check_bracket(label, t, t_in, w, padding, ur)
        assert bool((t[:, 1:] >= t[:, :-1]).all()), (label, "t_out must not decrease along a ray")
        check_cone(label, t, m, c, o, d, r)


def test_resample_den_threshold(lib):
    """One u on the midpoint of a bin of mass 8e-6 (den snaps to 1) and of one of mass 2e-5 (ordinary)."""
    s = ref.threshold_case()
    t, m, c = run_resample(lib, s["t"], s["w"], 0.0, s["u_rand"], s["o"], s["d"], s["r"], "resample/threshold")
    check_bracket("resample/threshold", t, s["t"], s["w"], 0.0, s["u_rand"])


# ------------------------------------------------------------------------------------------------- encodings
def enc_bound(device_units):
    return max(ref.ENC_FLOOR_UNITS, 2.0 * device_units)


@pytest.mark.parametrize("M", ref.IPE_M)
def test_ipe_encode(lib, M):
    mean, covs = ref.ipe_suite(M)
    rows = int(lib.load().pn_pad_rows(M))
    dm = G(mean)
    for name in ref.IPE_COVS:
        enc64, unit, y2, v2 = ref.ipe64(mean, covs[name])
        device = (torch.exp(-0.5 * G(v2)) * torch.sin(G(y2))).cpu()  # the device's own fp32 exp and sin on these arguments
        du = ref.units(device, enc64, unit)
        dc = G(covs[name])
        enc = torch.full((rows + EXTRA, 96), SENTINEL, dtype=torch.float32, device=dev())
        lib.call("pn_ipe_encode", M, dm.data_ptr(), dc.data_ptr(), enc.data_ptr(), st())
        got = logical(enc, M, f"ipe/{M}/{name}")  # rows M .. pn_pad_rows(M) are left alone too
        e = ref.units(got, enc64, unit)
        report_worst(f"encoding/ipe cov {name}: device torch.exp * torch.sin (units)", du)
        report_worst(f"encoding/ipe cov {name}: kernel (units, bound max(4, 2 x device))", e)
        assert e <= enc_bound(du), (M, name, "kernel", e, "device exp * sin", du)


@pytest.mark.parametrize("R", ref.VIEW_R)
def test_pos_enc_view(lib, R):
    x = ref.view_suite(R)
    enc64, unit, y2 = ref.view_enc64(x)
    du = ref.units(torch.sin(G(y2)).cpu(), enc64[:, 3:], unit[:, 3:])
    dx = G(x)
    ve = guarded(R, 27)
    lib.call("pn_pos_enc_view", R, dx.data_ptr(), ve.data_ptr(), st())
    got = logical(ve, R, f"view/{R}")
    assert torch.equal(got[:, :3], x), "identity columns must be bit-equal"
    e = ref.units(got, enc64, unit)
    report_worst("encoding/view: device torch.sin (units)", du)
    report_worst("encoding/view: kernel (units, bound max(4, 2 x device))", e)
    assert e <= enc_bound(du), (R, "kernel", e, "device sin", du)


# ------------------------------------------------------------------------------------------------- light rays
@pytest.mark.parametrize("Dn", ref.LIT_D)
def test_lit_rays(lib, Dn):
    out = torch.full((14 * Dn + 8,), 0x7b7b, dtype=torch.int16, device=dev())
    lib.call("pn_lit_rays", Dn, *ref.LIT_ARGS, out.data_ptr(), st())
    torch.cuda.synchronize()
    h = out.cpu().numpy().view(np.uint16)
    assert (h[14 * Dn:] == 0x7b7b).all(), "written beyond 14 D halves"
    got, want = h[:14 * Dn], ref.lit_rays_oracle_bits(Dn, *ref.LIT_ARGS)
    diff = got != want
    if diff.any():  # one fp16 ulp, and only where the fp64 value sits on a rounding tie (none at these sizes)
        ok = ref.near_half_tie(ref.lit_rays64(Dn, *ref.LIT_ARGS)) & (ref.half_ulps_apart(got, want) <= 1)
        assert not (diff & ~ok).any(), (Dn, np.nonzero(diff & ~ok)[0][:8], got[diff & ~ok][:8], want[diff & ~ok][:8])
    report_worst("lit rays: halves that differ from the oracle", float(diff.sum()))


# ------------------------------------------------------------------------------------------------- refusals
def test_refused_arguments_of_the_samplers():
    from pano_nerf_amd import _lib
    h = _lib.load()
    x = torch.zeros(2048, device=dev())
    p = x.data_ptr()
    assert h.pn_resample(4, 513, p, p, 0.01, None, p, p, p, p, p, p, None) == -2   # beyond PN_MAX_SAMPLES
    assert h.pn_resample(4, 8, None, p, 0.01, None, p, p, p, p, p, p, None) == -3  # null t_in
    assert h.pn_sample_env(4, 0, 8, p, p, p, p, p, p, p, None, p, p, p, None) == -1  # no light direction
    assert h.pn_lit_rays(1, 0.01, 0.0, 10.0, p, None) == -1                         # D - 1 divides
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0  # nothing was launched
