"""Emitter extraction on the GPU: pn_emitters.hip against the numpy restatement of tests/_emitters_ref.py - labels and counts
exactly, the records and the default threshold to the precision of the number formats - then batching, views,
determinism, the compositions with the model, the analytic probe, the energy bound and the errors.

Tolerances (from the number formats; both sides evaluate the header's formulas in fp64 on the same fp32 inputs - the
restatement is given the DEVICE's direction / solid-angle table - and round once).  ulp32(v) is the fp32 spacing at v.
  labels, count, pixels, peak, peak_index   exact: integers, and a maximum of identical fp64 values
  omega, flux, lum_flux    1 ulp32: every term is >= 0, so reordering an fp64 sum of n terms moves it by at most n 2^-53
                           relative, far below the final rounding to fp32, which can then differ by one ulp
  direction                2 x 2^-23 (two ulps of 1) per component, for components with |sum Y omega d| >= 0.5 lum_flux, where
                           cancellation loses at most one bit (asserted on the restatement; test_emitters_cpu.py asserts it for
                           the probes used here)
  distance                 2 ulp32: a ratio of two sums of non-negative terms
  angular_radius           2 ulp32: acos(1 - x), x = omega / 2 pi, has relative condition 1 / (2 x) with respect to the fp64
                           rounding of 1 - x, i.e. an error of 2^-53 / (2 x); the smallest pixel of the sizes used here (33 x 65)
                           has x > 3e-5, so the fp64 noise is below 2^-38 relative: far below an fp32 ulp
  spread                   2 ulp32 + 2^-40 rad: atan2(|d x u|, d . u) is well conditioned, but for a one-pixel component the true
                           angle is 0 and both sides return the rounding noise of the cross product of two nearly equal unit
                           vectors, at most 3 x 2^-52 per component: 2^-40 is a generous absolute floor for that and is 10^10
                           times smaller than a pixel
  default threshold        2 ulp32: log and exp may differ from numpy's in the last fp64 bit
Each comparison prints the worst value it saw."""
import functools
import math

import numpy as np
import pytest
import torch

import _emitters_ref as ref
from pano_nerf_amd import emitters as em

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def T(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).to(dev())


def N(x):
    return x.detach().cpu().numpy()


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def device_table(H, W):
    """the device's (dirs [H W, 3], omega [H W]) as numpy fp32: the inputs the kernels read"""
    from pano_nerf_amd import lighting
    dirs, omega = lighting.probe_directions(H, W, dev())
    return N(dirs), N(omega)


@functools.lru_cache(maxsize=None)
def mask_set(H, W):
    """(names, masks [P, H, W], probes [P, 3, H, W] fp32, flood-fill labels [P, H, W], counts [P]) of ref.masks(H, W)"""
    ms = ref.masks(H, W)
    names = list(ms)
    probes = np.stack([ref.probe_of_mask(ms[k], seed=i) for i, k in enumerate(names)])
    want = [ref.label_mask(ms[k]) for k in names]
    return names, np.stack([ms[k] for k in names]), probes, np.stack([w[0] for w in want]), np.array([w[1] for w in want], np.int32)


def check_labels(labels, count, want_labels, want_count, names, tag):
    got_l, got_c = N(labels), N(count)
    assert got_l.dtype == np.int32 and got_c.dtype == np.int32 and got_l.shape == want_labels.shape
    for p, name in enumerate(names):
        assert got_c[p] == want_count[p], (tag, name, int(got_c[p]), int(want_count[p]))
        assert np.array_equal(got_l[p], want_labels[p]), (tag, name)


# ------------------------------------------------------------------------------------------------------------ 1. labels
@pytest.mark.parametrize("size", ref.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labels_match_the_flood_fill(size):
    H, W = size
    names, _, probes, want_l, want_c = mask_set(H, W)
    labels, count = em.label_emitters(T(probes), ref.THRESHOLD)  # every mask of this size as one batch
    check_labels(labels, count, want_l, want_c, names, size)
    print(f"{H} x {W}: {len(names)} masks, counts {dict(zip(names, want_c.tolist()))}")
    # three different probes in one call equal three single calls, and two calls give the same bits
    pick = [names.index(k) for k in ("seam_blob", "random_0.4_1", "checkerboard")]
    for p in pick:
        l1, c1 = em.label_emitters(T(probes[p:p + 1]), ref.THRESHOLD)
        assert bits_equal(l1[0], labels[p]) and int(c1[0]) == int(count[p]), names[p]
    again = em.label_emitters(T(probes), ref.THRESHOLD)
    assert bits_equal(again[0], labels) and bits_equal(again[1], count)


def test_labels_64x128():
    H, W = 64, 128
    ms = ref.masks(H, W)
    names = ["random_0.4_0", "serpentine", "spiral", "comb", "nested_us", "random_0.1_0", "random_0.9_0"]
    probes = np.stack([ref.probe_of_mask(ms[k], seed=i) for i, k in enumerate(names)])
    want = [ref.label_mask(ms[k]) for k in names]
    labels, count = em.label_emitters(T(probes), ref.THRESHOLD)
    check_labels(labels, count, np.stack([w[0] for w in want]), np.array([w[1] for w in want]), names, "64x128")
    print("64 x 128 counts", {k: w[1] for k, w in zip(names, want)})


def test_special_pixels_and_thresholds():
    probe, want_mask = ref.special_probe()
    labels, count = em.label_emitters(T(probe[None]), ref.THRESHOLD)
    want_l, want_c = ref.label(probe, ref.THRESHOLD)
    assert np.array_equal(N(labels)[0] >= 0, want_mask) and np.array_equal(N(labels)[0], want_l) and int(count[0]) == want_c == 3
    # one threshold per probe, as a tensor; a number applies to all; a NaN threshold leaves nothing
    _, _, probes, _, _ = mask_set(8, 16)
    probes = probes[:4]
    thr = np.float32([1.0, 3.5, 6.0, np.nan])
    labels, count = em.label_emitters(T(probes), T(thr))
    for p in range(4):
        want_l, want_c = ref.label(probes[p], thr[p])
        assert np.array_equal(N(labels)[p], want_l) and int(count[p]) == want_c, p
    assert int(count[3]) == 0 and int(count[1]) > 0
    # +inf threshold: nothing is above it, not even +inf
    labels, count = em.label_emitters(T(probe[None]), float("inf"))
    assert int(count[0]) == 0 and (N(labels) == -1).all()
    # a negative threshold: every finite non-negative pixel is an emitter
    labels, count = em.label_emitters(T(probes[:1]), -1.0)
    assert int(count[0]) == 1 and (N(labels) == 0).all()


def test_views_are_read_in_place():
    """the permuted view light_probes returns ([P, H, W, 3] storage) gives the bits of its contiguous copy"""
    _, _, probes, want_l, want_c = mask_set(33, 65)
    pick = [0, 5, 9, 12]
    hwc = T(probes[pick].transpose(0, 2, 3, 1))
    view = hwc.permute(0, 3, 1, 2)
    assert not view.is_contiguous()
    lv, cv = em.label_emitters(view, ref.THRESHOLD)
    lc, cc = em.label_emitters(view.contiguous(), ref.THRESHOLD)
    assert bits_equal(lv, lc) and bits_equal(cv, cc)
    assert np.array_equal(N(lv), want_l[pick]) and np.array_equal(N(cv), want_c[pick])
    assert bits_equal(em.emitter_threshold(view), em.emitter_threshold(view.contiguous()))
    sv, sc = em.emitter_stats(view, lv, cv), em.emitter_stats(view.contiguous(), lc, cc)
    for k in sv:
        assert bits_equal(sv[k], sc[k]), k
    # a sliced view whose rows are not evenly spaced pixels is copied, not misread
    wide = T(np.concatenate([probes[pick], probes[pick]], -1))
    half = wide[..., :65]
    lh, ch = em.label_emitters(half, ref.THRESHOLD)
    assert bits_equal(lh, lc) and bits_equal(ch, cc)


# ----------------------------------------------------------------------------------------------------------- 2. records
def ulps(got, want):
    """|got - want| in units of the fp32 spacing at want (NaN where both are NaN -> 0)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - want) / ref.ulp32(np.where(both_nan, 1.0, want))
    return np.where(both_nan, 0.0, e)


def compare_records(got, want, count, tag, directions=True):
    """row 0 .. count - 1 of the device's dict (numpy, one probe) against the restatement's; prints the worst errors"""
    C = count
    for k in ("pixels", "peak_index"):
        assert np.array_equal(got[k][:C], want[k]), (tag, k)
    assert np.array_equal(got["peak"][:C], want["peak"].astype(np.float32)), (tag, "peak")
    worst = {}
    for k, n in (("omega", 1), ("flux", 1), ("lum_flux", 1), ("distance", 2), ("angular_radius", 2)):
        e = ulps(got[k][:C], want[k])
        worst[k] = float(e.max()) if e.size else 0.0
        assert np.isnan(got[k][:C]).tolist() == np.isnan(want[k]).tolist(), (tag, k)
        assert np.all(e <= n), (tag, k, worst[k])
    e = np.abs(got["spread"][:C].astype(np.float64) - want["spread"])
    lim = 2 * ref.ulp32(want["spread"]) + 2.0 ** -40
    worst["spread"] = float((e / lim).max()) if e.size else 0.0
    assert np.all(e <= lim), (tag, "spread", worst["spread"])
    if directions:
        ok = want["dir_norm"] >= 0.5
        assert ok.all(), (tag, "the restatement's components must be well conditioned", want["dir_norm"])
        e = np.abs(got["direction"][:C].astype(np.float64) - want["direction"]) / 2.0 ** -23
        worst["direction"] = float(e.max()) if e.size else 0.0
        assert np.all(e <= 2.0), (tag, "direction", worst["direction"])
    # rows beyond the count are zero
    for k in got:
        assert not got[k][C:].any(), (tag, k, "rows beyond the count")
    print(f"{tag}: {C} components; worst " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + " (ulp32; spread in units of its limit, direction in 2^-23)")


@pytest.mark.parametrize("size", [(16, 32), (33, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_records_match_the_restatement(size):
    H, W = size
    dirs, omega = device_table(H, W)
    made = [ref.blob_probe(H, W, seed) for seed in (0, 1)]
    a_probe, a_dist, _ = ref.analytic_probe(H, W)  # a third probe with fewer components: its rows beyond 2 must be zero
    probes = np.stack([m[0] for m in made] + [a_probe])
    dist = np.stack([m[1] for m in made] + [a_dist])
    tp = T(probes.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2)  # as light_probes returns them
    labels, count = em.label_emitters(tp, ref.THRESHOLD)
    got = em.emitter_stats(tp, labels, count, T(dist))
    Cmax = int(count.max())
    assert all(tuple(v.shape[:2]) == (3, Cmax) for v in got.values())
    assert got["pixels"].dtype == torch.int32 and got["peak_index"].dtype == torch.int32 and got["flux"].dtype == torch.float32
    blind = em.emitter_stats(tp, labels, count)
    for p in range(3):
        want_l, want_c = ref.label(probes[p], ref.THRESHOLD)
        assert np.array_equal(N(labels)[p], want_l) and int(count[p]) == want_c
        want = ref.stats(probes[p], want_l, want_c, dirs, omega, dist[p])
        compare_records({k: N(v)[p] for k, v in got.items()}, want, want_c, f"{H} x {W} probe {p}")
        # without a distance map: NaN distances, everything else the same bits
        assert np.isnan(N(blind["distance"])[p, :want_c]).all() and not N(blind["distance"])[p, want_c:].any()
        for k in got:
            if k != "distance":
                assert bits_equal(blind[k][p], got[k][p]), k
    assert int(count[2]) == 2 and Cmax > 2
    # [P, 1, H, W] distances are the same; two calls give the same bits; one probe alone gives its rows of the batch
    again = em.emitter_stats(tp, labels, count, T(dist)[:, None])
    alone = em.emitter_stats(tp[1:2], labels[1:2], count[1:2], T(dist)[1:2])
    for k in got:
        assert bits_equal(again[k], got[k]), k
        assert bits_equal(alone[k][0], got[k][1, :int(count[1])]), k


def test_records_of_many_small_components():
    """a 0.1-density random mask: over a hundred components, most of a pixel or two (one wave each): the exact fields and the
    sums (a larger component's directions may cancel here, so `direction` is checked where the restatement is well
    conditioned)"""
    H, W = 33, 65
    dirs, omega = device_table(H, W)
    names, _, probes, want_l, want_c = mask_set(H, W)
    p = names.index("random_0.1_0")
    dist = (1.0 + np.random.default_rng(5).random((H, W))).astype(np.float32)
    tp = T(probes[p:p + 1])
    labels, count = em.label_emitters(tp, ref.THRESHOLD)
    got = em.emitter_stats(tp, labels, count, T(dist[None]))
    want = ref.stats(probes[p], want_l[p], int(want_c[p]), dirs, omega, dist)
    assert int(want_c[p]) > 100 and (want["pixels"] == 1).sum() > 10
    compare_records({k: N(v)[0] for k, v in got.items()}, want, int(want_c[p]), "33 x 65 random 0.1", directions=False)
    ok = want["dir_norm"] >= 0.5
    e = np.abs(N(got["direction"])[0][ok].astype(np.float64) - want["direction"][ok]) / 2.0 ** -23
    print(f"direction of the {int(ok.sum())} well-conditioned components: worst {e.max():.2f} x 2^-23")
    assert np.all(e <= 2.0)


def test_ring_falls_back_to_the_peak_pixel():
    """A closed band around the pole axis.  Where the restatement (on the device's table) finds the weighted directions
    cancelled below 1e-12 lum_flux, the direction must be the peak pixel's, bit for bit; with directions held in fp32 a
    bright band cancels only to about 1e-8, so the rule is also exercised where it surely fires: a band of zero luminance
    under a negative threshold (sum = 0 exactly), whose peak pixel - every pixel ties - is the band's first."""
    H, W = 16, 32
    dirs, omega = device_table(H, W)
    probe = ref.ring_probe(H, W)
    dark = np.full_like(probe, -5.0)
    dark[:, H // 2 - 1:H // 2 + 1, :] = 0.0
    tp = T(np.stack([probe, dark]))
    thr = T(np.float32([ref.THRESHOLD, -1.0]))
    labels, count = em.label_emitters(tp, thr)
    got = {k: N(v) for k, v in em.emitter_stats(tp, labels, count).items()}
    assert N(count).tolist() == [1, 1]
    first = (H // 2 - 1) * W
    for p, (img, t) in enumerate(((probe, ref.THRESHOLD), (dark, -1.0))):
        want_l, want_c = ref.label(img, t)
        want = ref.stats(img, want_l, want_c, dirs, omega)
        assert np.array_equal(N(labels)[p], want_l) and want_c == 1 and got["pixels"][p, 0] == 2 * W
        assert got["peak_index"][p, 0] == first == want["peak_index"][0]
        print(f"band {p}: |sum Y omega d| / lum_flux = {want['dir_norm'][0]:.3e}, fallback {bool(want['fallback'][0])}")
        if want["fallback"][0]:
            assert np.array_equal(got["direction"][p, 0], dirs[first]), p
        else:
            assert want["dir_norm"][0] > 1e-11, "within a factor of 10 of the rule: the two sides may decide differently"
            assert abs(np.linalg.norm(got["direction"][p, 0].astype(np.float64)) - 1.0) < 1e-6
    assert ref.stats(dark, *ref.label(dark, -1.0), dirs, omega)["fallback"][0]  # the second band does exercise the rule


# --------------------------------------------------------------------------------------------------------- 3. threshold
def test_default_threshold():
    H, W = 16, 32
    _, omega = device_table(H, W)
    a_probe, _, _ = ref.analytic_probe(H, W)
    b_probe, _ = ref.blob_probe(H, W)
    odd = b_probe.copy()
    odd[:, 0, 0], odd[:, 3, 4], odd[0, 5, 5], odd[:, 7, 7] = np.nan, np.inf, -np.inf, 0.0  # skipped, skipped, skipped, clamped to 1e-6
    neg = b_probe.copy()
    neg[:, 2, :] = -3.0  # negative luminance: clamped
    probes = np.stack([a_probe, b_probe, odd, neg, np.full_like(a_probe, np.nan)])
    got = N(em.emitter_threshold(T(probes)))
    want = np.array([ref.threshold(p, omega) for p in probes], np.float64)
    e = ulps(got[:4], want[:4])
    print("default thresholds", got.tolist(), "worst", float(e.max()), "ulp32")
    assert np.all(e <= 2) and np.isnan(got[4]) and np.isnan(want[4])
    for ratio in (1.0, 20.0):
        got = N(em.emitter_threshold(T(probes[:2]), ratio))
        assert np.all(ulps(got, [ref.threshold(p, omega, ratio) for p in probes[:2]]) <= 2)
    # 33 x 65: 2145 pixels, the last pass of the 1024 threads is partial
    _, omega = device_table(33, 65)
    p = ref.blob_probe(33, 65)[0]
    assert ulps(N(em.emitter_threshold(T(p[None])))[0], ref.threshold(p, omega)) <= 2
    # under a NaN threshold nothing is an emitter
    assert int(em.label_emitters(T(probes[4:5]), em.emitter_threshold(T(probes[4:5])))[1][0]) == 0


# ------------------------------------------------------------------------------------------------ 4. the analytic probe
@pytest.mark.parametrize("size", [(16, 32), (64, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_analytic_probe(size):
    H, W = size
    a = ref.ANALYTIC
    probe, dist, axes = ref.analytic_probe(H, W)
    pos = np.asarray(a["position"])
    lists = em.emitters_from_probes(T(probe[None]), T(pos[None]), T(dist[None]))
    assert len(lists) == 1 and len(lists[0]) == 2
    es = lists[0]
    assert es[0].lum_flux > es[1].lum_flux and [e.probe for e in es] == [0, 0]
    diag = math.sqrt(2.0) * math.pi / H
    for rank, e in enumerate(es):
        ang = math.acos(min(1.0, float(e.direction @ axes[rank])))
        print(f"{H} x {W} disc {rank}: {e.pixels} pixels, {ang:.4f} rad off axis (pixel diagonal {diag:.4f}), distance {e.distance}")
        assert ang <= diag
        assert e.distance == a["distance"][rank]
        assert np.linalg.norm(e.position - (pos + axes[rank] * a["distance"][rank])) <= a["distance"][rank] * diag
        np.testing.assert_allclose(e.intensity, e.flux * a["distance"][rank] ** 2, rtol=1e-12)  # fp64 on the host: to rounding
        assert abs(e.radius - e.distance * math.sin(e.angular_radius)) < 1e-12
    # against the restatement on the device's table, default threshold included
    dirs, omega = device_table(H, W)
    want_l, want_c = ref.label(probe, ref.threshold(probe, omega))
    want = ref.stats(probe, want_l, want_c, dirs, omega, dist)
    order = np.argsort(-want["lum_flux"], kind="stable")
    assert [e.label for e in es] == order.tolist()
    for e, c in zip(es, order):
        assert e.pixels == want["pixels"][c] and ulps(e.lum_flux, want["lum_flux"][c]) <= 1
    # selection: a solid-angle floor between the two discs' keeps the larger, max_emitters cuts, no distance -> NaN lights
    mid = 0.5 * (es[0].omega + es[1].omega)
    big = em.emitters_from_probes(T(probe[None]), pos[None], T(dist[None]), min_solid_angle=mid)[0]
    assert [e.label for e in big] == [es[0].label if es[0].omega > es[1].omega else es[1].label]
    assert [e.label for e in em.emitters_from_probes(T(probe[None]), pos[None], max_emitters=1)[0]] == [es[0].label]
    blind = em.emitters_from_probes(T(probe[None]), pos[None])[0]
    assert all(np.isnan(e.distance) and np.isnan(e.position).all() and np.isnan(e.intensity).all() for e in blind)
    with pytest.raises(ValueError, match="has no distance"):
        em.to_point_lights(blind)


# ------------------------------------------------------------------------------------------------------- 5. the bound
@pytest.mark.parametrize("size", [(16, 32), (64, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_energy_bound(size):
    """| E_all(n) - E_background(n) - sum_i lum_flux_i relu(n . direction_i) | <= sum_i lum_flux_i 2 sin(spread_i / 2), with E
    from lighting.irradiance (the channel mean of its RGB, as the luminance is) on the probe and on the probe with its
    emitters blacked out"""
    from pano_nerf_amd import lighting
    H, W = size
    probe, dist, _ = ref.analytic_probe(H, W)
    tp = T(probe[None])
    labels, count = em.label_emitters(tp, em.emitter_threshold(tp))
    rec = {k: N(v)[0].astype(np.float64) for k, v in em.emitter_stats(tp, labels, count, T(dist[None])).items()}
    n = np.random.default_rng(1).standard_normal((64, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    background = torch.where(labels[:, None] >= 0, torch.zeros_like(tp), tp)
    e_all = N(lighting.irradiance(tp, T(n)))[0].astype(np.float64).sum(1) / 3.0
    e_bg = N(lighting.irradiance(background, T(n)))[0].astype(np.float64).sum(1) / 3.0
    cos = n @ rec["direction"].T
    lights = (np.where(cos < 0, 0.0, cos) * rec["lum_flux"]).sum(1)
    gap = np.abs(e_all - e_bg - lights)
    bound = float((rec["lum_flux"] * 2 * np.sin(rec["spread"] / 2)).sum())
    print(f"{H} x {W}: worst gap {gap.max():.4f}, bound {bound:.4f}")
    assert int(count[0]) == 2 and (gap <= bound).all() and gap.max() > 0.01 * bound


# ------------------------------------------------------------------------------------------------------ 6. compositions
@functools.lru_cache(maxsize=None)
def model():
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    m = pn.PanoMipNeRF(num_samples=16, rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    m.mlp.load_state_dict(orc.init_params(4, 5))
    return m.to(dev())


POSITIONS = np.float32([[0.3, 0.4, -0.2], [-0.4, 0.5, 0.3], [0.0, -0.1, 0.1]])


@functools.lru_cache(maxsize=None)
def rendered():
    """(probes, distance) of the small random model at 8 x 16, rendered once"""
    return em.probe_rgbd(model(), T(POSITIONS), 8, 16)


def test_probe_rgbd_is_light_probes_and_shadow_maps():
    from pano_nerf_amd import lighting, relight as rl
    probes, dist = rendered()
    assert tuple(probes.shape) == (3, 3, 8, 16) and tuple(dist.shape) == (3, 8, 16) and not probes.is_contiguous()
    assert bits_equal(probes, lighting.light_probes(model(), T(POSITIONS), 8, 16))
    assert bits_equal(dist, rl.shadow_maps(model(), T(POSITIONS), 8, 16, kind="pano"))
    p2, d2 = em.probe_rgbd(model(), T(POSITIONS), 8, 16, near=0.05, far=6.0, chunk_rays=50)
    assert bits_equal(p2, lighting.light_probes(model(), T(POSITIONS), 8, 16, 0.05, 6.0, 50))
    assert bits_equal(d2, rl.shadow_maps(model(), T(POSITIONS), 8, 16, "pano", 0.05, 6.0, 50))
    assert bool(torch.isfinite(probes).all()) and bool(torch.isfinite(dist).all())


def threshold_of(probes):
    """a threshold that splits the random model's smooth probes into emitters and background: the mean luminance"""
    return float(probes.mean())


def test_extract_emitters_is_the_composition():
    probes, dist = rendered()
    thr = threshold_of(probes)
    got = em.extract_emitters(model(), T(POSITIONS), size=(8, 16), threshold=thr, max_emitters=4)
    assert bits_equal(got["probes"], probes) and bits_equal(got["distance"], dist)
    labels, count = em.label_emitters(probes, thr)
    assert bits_equal(got["labels"], labels) and bits_equal(got["count"], count) and int(count.sum()) > 0
    hand = em.emitters_from_probes(probes, T(POSITIONS), dist, threshold=thr, max_emitters=4)
    rec = {k: N(v) for k, v in em.emitter_stats(probes, labels, count, dist).items()}
    assert len(got["emitters"]) == len(hand) == 3
    for p, (a, b) in enumerate(zip(got["emitters"], hand)):
        assert len(a) == len(b) == min(4, int(count[p]))
        assert [e.lum_flux for e in a] == sorted((e.lum_flux for e in a), reverse=True)
        for x, y in zip(a, b):
            assert (x.probe, x.label) == (y.probe, y.label) == (p, x.label)
            for k in em.Emitter.__slots__:
                assert np.array_equal(np.asarray(getattr(x, k)), np.asarray(getattr(y, k)), equal_nan=True), k
            for k in ref.FIELDS:  # the record is emitter_stats' row
                assert np.array_equal(np.asarray(getattr(x, k), np.float64), rec[k][p, x.label].astype(np.float64)), k
            np.testing.assert_allclose(x.position, POSITIONS[p].astype(np.float64) + x.direction * x.distance, atol=1e-12)
    # the default threshold is emitter_threshold's
    auto = em.extract_emitters(model(), T(POSITIONS), size=(8, 16))
    la, ca = em.label_emitters(probes, em.emitter_threshold(probes))
    assert bits_equal(auto["labels"], la) and bits_equal(auto["count"], ca)


def dilate(mask, grow):
    m = mask.copy()
    for _ in range(grow):
        out = m.copy()
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                s = np.roll(m, dj, axis=-1)
                if di == 1:
                    s = np.concatenate([np.zeros_like(s[..., :1, :]), s[..., :-1, :]], -2)
                elif di == -1:
                    s = np.concatenate([s[..., 1:, :], np.zeros_like(s[..., :1, :])], -2)
                out |= s
        m = out
    return m


def test_residual_probes_are_fill_holes():
    from pano_nerf_amd import views
    probes, dist = rendered()
    labels, count = em.label_emitters(probes, threshold_of(probes))
    gone = N(labels) >= 0
    assert gone.any() and not gone.all()
    cam = views.pano_camera(8, 16)
    for distance in (dist, None):
        got = em.residual_probes(probes, labels, distance)
        assert bits_equal(got, views.fill_holes(probes, distance, labels < 0, cam)["image"])
        keep = T(~gone, torch.bool)[:, None].expand(-1, 3, -1, -1)
        assert bits_equal(got[keep], probes[keep])  # known pixels keep their bits
        assert not bits_equal(got, probes.contiguous()) and bool(torch.isfinite(got).all())
    for grow in (1, 2):
        known = ~dilate(gone, grow)
        assert known.sum() < (~gone).sum()
        got = em.residual_probes(probes, labels, dist, grow=grow)
        assert bits_equal(got, views.fill_holes(probes, dist, T(known, torch.bool), cam)["image"]), grow
    # the seam: a removed pixel in column 0 takes column W - 1 with it
    one = torch.full((1, 8, 16), -1, dtype=torch.int32, device=dev())
    one[0, 3, 0] = 0
    want = np.zeros((1, 8, 16), bool)
    want[0, 2:5, [15, 0, 1]] = True
    got = em.residual_probes(probes[:1], one, grow=1)
    changed = N((got != probes[:1]).any(1))
    assert not changed[~want].any()
    with pytest.raises(ValueError, match="grow"):
        em.residual_probes(probes, labels, grow=-1)


def test_point_lights_pack_and_cast_shadows(tmp_path):
    from pano_nerf_amd import relight as rl
    probes, dist = rendered()
    lists = em.emitters_from_probes(probes, POSITIONS, dist, threshold=threshold_of(probes), max_emitters=2)
    lights = em.to_point_lights(lists, standoff=0.05)
    assert 1 <= len(lights) <= 6
    packed = rl.pack_lights(lights, dev())
    assert tuple(packed.shape) == (len(lights), 16) and np.array_equal(N(packed), rl.light_rows(lights))
    flat = [e for es in lists for e in es]
    for e, row in zip(flat, N(packed)):
        np.testing.assert_allclose(row[:3], e.position - 0.05 * e.direction, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(row[3:6], e.flux * e.distance ** 2, rtol=1e-6)
        assert row[11] == np.float32(e.radius)
    maps = rl.shadow_maps(model(), lights, 8, 16)
    assert tuple(maps.shape) == (len(lights), 8, 16) and bool(torch.isfinite(maps).all())
    path = str(tmp_path / "lights.json")
    em.save_lights(path, lists)
    np.testing.assert_allclose(rl.light_rows(em.load_lights(path)), rl.light_rows(em.to_point_lights(lists)), rtol=2e-7)


# ----------------------------------------------------------------------------------------------------------- 7. errors
def test_python_errors():
    probes = T(ref.analytic_probe(8, 16)[0][None].repeat(2, 0))
    labels, count = em.label_emitters(probes, 1.0)
    for bad in (torch.ones(3, device=dev()), torch.ones(2, 1, device=dev()), torch.ones(1, device=dev())):
        with pytest.raises(ValueError, match="threshold"):
            em.label_emitters(probes, bad)
    with pytest.raises(RuntimeError, match="HIP device only"):
        em.label_emitters(probes, torch.ones(2))
    with pytest.raises(ValueError, match="threshold"):
        em.label_emitters(probes, "bright")
    for bad in (T(np.zeros((2, 3, 1, 16))), T(np.zeros((2, 3, 8, 1))), T(np.zeros((2, 4, 8, 16))), T(np.zeros((3, 8, 16)))):
        with pytest.raises(ValueError):
            em.label_emitters(bad, 1.0)
        with pytest.raises(ValueError):
            em.emitter_threshold(bad)
    for bad_labels in (labels[:1], labels[:, :4], labels.to(torch.int64), labels.float(), labels.view(2, 16, 8), N(labels)):
        with pytest.raises(ValueError, match="labels"):
            em.emitter_stats(probes, bad_labels, count)
        with pytest.raises(ValueError, match="labels"):
            em.residual_probes(probes, bad_labels)
    with pytest.raises(RuntimeError, match="HIP device only"):
        em.emitter_stats(probes, labels.cpu(), count)
    for bad_count in (count[:1], count.to(torch.int64), [1, 1]):
        with pytest.raises(ValueError, match="count"):
            em.emitter_stats(probes, labels, bad_count)
    for bad_dist in (torch.ones(2, 8, 8, device=dev()), torch.ones(1, 8, 16, device=dev()), N(probes[:, 0])):
        with pytest.raises(ValueError, match="distance"):
            em.emitter_stats(probes, labels, count, bad_dist)
    with pytest.raises(RuntimeError, match="HIP device only"):
        em.emitter_stats(probes, labels, count, torch.ones(2, 8, 16))
    with pytest.raises(ValueError, match="positions"):
        em.emitters_from_probes(probes, np.zeros((3, 3)))
    with pytest.raises(RuntimeError, match="HIP device only"):
        em.probe_rgbd(model(), torch.zeros(1, 3), 8, 16)
    with pytest.raises(ValueError, match="positions"):
        em.probe_rgbd(model(), torch.zeros(3, device=dev()), 8, 16)
    # no emitter at all: empty records, empty lists
    none = em.label_emitters(probes, 1e9)
    stats = em.emitter_stats(probes, *none)
    assert int(none[1].sum()) == 0 and tuple(stats["flux"].shape) == (2, 0, 3) and tuple(stats["pixels"].shape) == (2, 0)
    assert em.emitters_from_probes(probes, np.zeros((2, 3)), threshold=1e9) == [[], []]


def test_error_codes():
    from pano_nerf_amd import _lib
    lib = _lib.load()
    P, H, W = 2, 8, 16
    HW = H * W
    f = lambda *s: torch.ones(*s, device=dev())
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev())
    x, omega, dirs, thr, dist = f(P, 3, H, W), f(HW), f(HW, 3), f(P), f(P, HW)
    parent, roots, flags, prefix, count = i32(P, HW), i32(P, HW), i32(P, HW), i32(P, HW), i32(P)
    order, starts = torch.arange(P * HW, device=dev()), torch.zeros(P * 2 + 1, dtype=torch.int64, device=dev())
    outs = [i32(P, 2), f(P, 2), f(P, 2, 3), f(P, 2), f(P, 2, 3), f(P, 2), i32(P, 2), f(P, 2), f(P, 2), f(P, 2)]
    st = _lib.stream(dev())
    p = lambda t: None if t is None else t.data_ptr()
    view = (3 * HW, HW, 1)
    OK, SHAPE, NULL = 0, -1, -3

    def threshold(**kw):
        a = dict(P=P, H=H, W=W, x=x, omega=omega, ratio=8.0, out=thr)
        a.update(kw)
        return lib.pn_emitter_threshold(a["P"], a["H"], a["W"], p(a["x"]), *view, p(a["omega"]), a["ratio"], p(a["out"]), st)

    def labels(**kw):
        a = dict(P=P, H=H, W=W, x=x, thr=thr, parent=parent, roots=roots, flags=flags)
        a.update(kw)
        return lib.pn_emitter_labels(a["P"], a["H"], a["W"], p(a["x"]), *view, p(a["thr"]), p(a["parent"]), p(a["roots"]),
                                     p(a["flags"]), st)

    def compact(**kw):
        a = dict(P=P, H=H, W=W, prefix=prefix, labels=roots, count=count)
        a.update(kw)
        return lib.pn_emitter_compact(a["P"], a["H"], a["W"], p(a["prefix"]), p(a["labels"]), p(a["count"]), st)

    def stats(**kw):
        a = dict(P=P, H=H, W=W, x=x, dirs=dirs, omega=omega, dist=dist, C=2, N=P * HW, order=order, starts=starts, outs=outs)
        a.update(kw)
        return lib.pn_emitter_stats(a["P"], a["H"], a["W"], p(a["x"]), *view, p(a["dirs"]), p(a["omega"]), p(a["dist"]), a["C"],
                                    a["N"], p(a["order"]), p(a["starts"]), *(p(t) for t in a["outs"]), st)

    shapes = (dict(P=0), dict(P=-1), dict(P=1 << 25), dict(H=1), dict(W=1), dict(H=0), dict(W=-2), dict(H=1 << 15, W=1 << 15))
    for call in (threshold, labels, compact, stats):
        assert call() == OK, call.__name__
        for kw in shapes:
            assert call(**kw) == SHAPE, (call.__name__, kw)
    for ratio in (0.0, -8.0, float("nan"), float("inf")):
        assert threshold(ratio=ratio) == SHAPE, ratio
    for kw in (dict(C=-1), dict(C=HW + 1), dict(N=-1), dict(N=P * HW + 1)):
        assert stats(**kw) == SHAPE, kw
    for call, names in ((threshold, ("x", "omega", "out")), (labels, ("x", "thr", "parent", "roots", "flags")),
                        (compact, ("prefix", "labels", "count")), (stats, ("x", "dirs", "omega", "order", "starts"))):
        for name in names:
            assert call(**{name: None}) == NULL, (call.__name__, name)
    for k in range(len(outs)):
        assert stats(outs=outs[:k] + [None] + outs[k + 1:]) == NULL, k
    assert stats(dist=None) == OK and stats(C=0, order=None, starts=None, outs=[None] * 10) == OK
    assert stats(N=0, order=None) == OK
    torch.cuda.synchronize()
