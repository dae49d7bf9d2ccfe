"""The emitter contract on the CPU: the fp64 restatement (tests/_emitters_ref.py) on patterns whose answer is known, the
analytic probe, the energy bound, the conditions the GPU comparison relies on, and the host-side half of
pano_nerf_amd.emitters (validation, Emitter records, point lights, the JSON file).  No GPU."""
import json
import math

import numpy as np
import pytest
import torch

import _emitters_ref as ref
from pano_nerf_amd import emitters as em
from pano_nerf_amd import relight as rl


# ----------------------------------------------------------------------------------------------------- the restatement
def test_known_patterns():
    want = {"seam_blob": 1, "seam_diagonal": 1, "seam_antidiagonal": 1, "diagonal": 1, "row0_opposite": 2, "pole_to_pole": 2,
            "serpentine": 1, "spiral": 1, "comb": 1, "checkerboard": 1, "all": 1, "none": 0}
    for H, W in ref.SIZES + ((64, 128),):
        ms = ref.masks(H, W)
        for name, m in ms.items():
            labels, count = ref.label_mask(m)
            assert ((labels >= 0) == m).all(), (H, W, name)
            if name in want:
                assert count == want[name], (H, W, name, count)
            # numbered by smallest pixel index: the first pixels of the components, in label order, ascend
            first = [int(np.flatnonzero(labels.reshape(-1) == c)[0]) for c in range(count)]
            assert first == sorted(first), (H, W, name)
    assert ref.label_mask(ref.masks(33, 65)["nested_us"])[1] == 16 and ref.label_mask(ref.masks(8, 16)["nested_us"])[1] == 4
    assert {"serpentine", "spiral", "comb", "nested_us"} <= set(ref.masks(5, 7)) and "row0_opposite" not in ref.masks(2, 3)
    # the long single components really are long and thin
    assert ref.serpentine(33, 65).sum() == 17 * 63 + 16 and ref.spiral(33, 65).sum() > 1000


def test_wrap_and_poles_by_hand():
    m = np.zeros((4, 6), bool)
    m[1, 5] = m[2, 0] = True  # a diagonal across the seam
    assert ref.label_mask(m)[1] == 1
    m[:] = False
    m[1, 4] = m[2, 0] = True  # one column short of it
    assert ref.label_mask(m)[1] == 2
    m[:] = False
    m[0, 2] = m[3, 2] = True  # the same column at both poles
    assert ref.label_mask(m)[1] == 2
    m[:] = False
    m[0, :] = True            # a full ring is one component, numbered 0, and the row below joins it
    m[1, 3] = True
    labels, count = ref.label_mask(m)
    assert count == 1 and labels[1, 3] == 0


def test_special_pixels():
    probe, want = ref.special_probe()
    got = ref.emitter_mask(probe, ref.THRESHOLD)
    assert (got == want).all()
    labels, count = ref.label(probe, ref.THRESHOLD)
    assert count == 3 and labels[3, 0] == labels[3, 7] and labels[0, 1] == 0 and labels[1, 4] == 1


def test_default_threshold_keeps_the_second_lamp():
    """the issue's example: on the 16 x 32 analytic probe eight times the ARITHMETIC mean nearly loses the radiance-20 lamp; the
    geometric mean does not"""
    probe, _, _ = ref.analytic_probe(16, 32)
    _, omega = ref.table(16, 32)
    y, w = ref.luminance(probe).reshape(-1), omega.astype(np.float64)
    arithmetic = 8.0 * (y * w).sum() / w.sum()
    thr = float(ref.threshold(probe, omega))
    assert 14.0 < arithmetic < 20.0 and 1.0 < thr < 5.0
    assert abs(thr - 8.0 * math.exp((w * np.log(y)).sum() / w.sum())) < 1e-6 * thr
    bad = probe.copy()
    bad[:, 0, 0] = np.nan
    bad[:, 0, 1] = np.inf
    assert np.isfinite(ref.threshold(bad, omega))
    assert np.isnan(ref.threshold(np.full_like(probe, np.nan), omega))


@pytest.mark.parametrize("size", [(16, 32), (64, 128)])
def test_analytic_probe(size):
    H, W = size
    a = ref.ANALYTIC
    probe, dist, axes = ref.analytic_probe(H, W)
    dirs, omega = ref.table(H, W)
    labels, count = ref.label(probe, ref.threshold(probe, omega))
    assert count == 2
    rec = ref.stats(probe, labels, count, dirs, omega, dist)
    order = np.argsort(-rec["lum_flux"], kind="stable")
    diag = math.sqrt(2.0) * math.pi / H
    for rank, c in enumerate(order):  # brightest first = the radiance-50 disc
        ang = math.acos(min(1.0, float(rec["direction"][c] @ axes[rank])))
        assert ang <= diag, (size, rank, ang, diag)
        assert rec["distance"][c] == a["distance"][rank]
        pos, radius, intensity = ref.light_of(rec, c, a["position"])
        truth = np.asarray(a["position"]) + axes[rank] * a["distance"][rank]
        assert np.linalg.norm(pos - truth) <= a["distance"][rank] * diag
        np.testing.assert_allclose(intensity, rec["flux"][c] * a["distance"][rank] ** 2, rtol=1e-6)
        # the cap of equal solid angle is about the disc (pixelisation moves it by a pixel at most)
        assert abs(rec["angular_radius"][c] - a["radius"][rank]) <= math.pi / H
        assert rec["spread"][c] <= a["radius"][rank] + diag
    # the first disc lies across the seam
    assert (labels[:, 0] == labels[:, W - 1]).all() and (labels[:, 0] >= 0).any()


@pytest.mark.parametrize("size", [(16, 32), (64, 128)])
def test_energy_bound(size):
    H, W = size
    probe, dist, _ = ref.analytic_probe(H, W)
    dirs, omega = ref.table(H, W)
    labels, count = ref.label(probe, ref.threshold(probe, omega))
    rec = ref.stats(probe, labels, count, dirs, omega, dist)
    n = np.random.default_rng(1).standard_normal((64, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    gap, bound = ref.energy_gap_and_bound(probe, labels, rec, n, dirs, omega)
    print(f"{H} x {W}: worst gap {gap.max():.4f}, bound {bound:.4f}")
    assert (gap <= bound).all() and gap.max() > 0.01 * bound  # holds, and is not vacuous


def test_conditions_of_the_gpu_comparison():
    """the record probes: every component's weighted directions add up (|sum Y omega d| >= 0.5 lum_flux, where cancellation
    costs at most one bit), the inputs are non-negative, the distance map has every kind of bad pixel; the ring's do not"""
    for H, W in ((16, 32), (33, 65)):
        probe, dist = ref.blob_probe(H, W)
        assert (probe >= 0).all() and np.isfinite(probe).all()
        dirs, omega = ref.table(H, W)
        labels, count = ref.label(probe, ref.THRESHOLD)
        rec = ref.stats(probe, labels, count, dirs, omega, dist)
        assert count >= 5 and (rec["dir_norm"] >= 0.5).all() and not rec["fallback"].any(), rec["dir_norm"]
        assert (labels[:, 0] >= 0).any() and (labels[:, 0] == labels[:, W - 1])[labels[:, 0] >= 0].all()  # one across the seam
        assert 1 in rec["pixels"]
        inside = dist[labels >= 0]
        assert (inside == 0).any() and np.isinf(inside).any() and np.isnan(inside).any() and (inside < 0).any()
        two = np.flatnonzero(rec["peak"] == 64.0)
        assert len(two) == 1
        pix = np.flatnonzero((ref.luminance(probe).reshape(-1) == 64.0) & (labels.reshape(-1) == two[0]))
        assert len(pix) == 2 and rec["peak_index"][two[0]] == pix.min()
    probe = ref.ring_probe()
    dirs, omega = ref.table(16, 32)
    labels, count = ref.label(probe, ref.THRESHOLD)
    rec = ref.stats(probe, labels, count, dirs, omega)
    assert count == 1 and rec["dir_norm"][0] < 1e-6 and rec["peak_index"][0] == 7 * 32 and np.isnan(rec["distance"][0])


# ------------------------------------------------------------------------------------------------ the host side of the module
def records(H=16, W=32):
    probe, dist, axes = ref.analytic_probe(H, W)
    dirs, omega = ref.table(H, W)
    labels, count = ref.label(probe, ref.threshold(probe, omega))
    rec = ref.stats(probe, labels, count, dirs, omega, dist)
    rec32 = {k: (rec[k].astype(np.float32) if rec[k].dtype == np.float64 else rec[k]) for k in ref.FIELDS}
    return rec, [em.Emitter(0, c, {k: rec32[k][c] for k in ref.FIELDS}, ref.ANALYTIC["position"]) for c in range(count)]


def test_emitter_records_and_point_lights():
    rec, es = records()
    for c, e in enumerate(es):
        pos, radius, intensity = ref.light_of(rec, c, ref.ANALYTIC["position"])
        assert e.probe == 0 and e.label == c and e.pixels == rec["pixels"][c] and e.peak_index == rec["peak_index"][c]
        np.testing.assert_allclose(e.position, pos, rtol=0, atol=1e-15)
        np.testing.assert_allclose(e.intensity, intensity, rtol=1e-15)
        assert abs(e.radius - radius) <= 1e-15 and "Emitter(probe=0" in repr(e)
    with pytest.raises(AttributeError):
        es[0].colour = 1  # slotted, like PointLight
    lights = em.to_point_lights([es])  # a list of lists flattens
    assert len(lights) == 2 and all(isinstance(x, rl.PointLight) for x in lights)
    rows = rl.light_rows(lights)
    assert rows.shape == (2, 16)
    for e, row in zip(es, rows):
        assert np.array_equal(row[0:3], e.position.astype(np.float32)) and np.array_equal(row[3:6], e.intensity.astype(np.float32))
        assert row[11] == np.float32(e.radius) and not row[6:11].any()
    back = em.to_point_lights(es, standoff=0.25, r_min=0.05)
    for e, x in zip(es, back):
        np.testing.assert_allclose(x.position, e.position - 0.25 * e.direction, atol=1e-15)
        assert x.r_min == 0.05
        # moved towards the probe: nearer to it by the standoff
        p0 = np.asarray(ref.ANALYTIC["position"])
        assert abs(np.linalg.norm(e.position - p0) - np.linalg.norm(x.position - p0) - 0.25) < 1e-6
    with pytest.raises(ValueError, match="standoff"):
        em.to_point_lights(es, standoff=-1.0)
    blind = records()[1]
    blind[1].distance = float("nan")
    with pytest.raises(ValueError, match="emitter 1 of probe 0 has no distance"):
        em.to_point_lights(blind)


def test_lights_file(tmp_path):
    _, es = records()
    path = str(tmp_path / "lights.json")
    em.save_lights(path, es)
    with open(path) as fh:
        doc = json.load(fh)
    assert "not candela" in doc["asset"]["units"] and doc["asset"]["layout"] == "KHR_lights_punctual"
    assert len(doc["lights"]) == 2
    for e, entry in zip(es, doc["lights"]):
        assert entry["type"] == "point" and entry["probe"] == 0 and max(entry["color"]) == 1.0
        assert entry["intensity"] == float(e.intensity.max()) and entry["solid_angle"] == e.omega
        assert entry["position"] == e.position.tolist() and entry["direction"] == e.direction.tolist() and entry["radius"] == e.radius
    got, want = rl.light_rows(em.load_lights(path)), rl.light_rows(em.to_point_lights(es))
    np.testing.assert_allclose(got, want, rtol=2e-7, atol=0)  # color x intensity rounds once more than intensity itself
    blind = records()[1]
    blind[0].distance, blind[0].intensity = float("nan"), np.full(3, np.nan)
    with pytest.raises(ValueError, match="no finite intensity"):
        em.save_lights(path, blind)


def test_cpu_tensors_and_shapes_raise():
    probes = torch.rand(2, 3, 8, 16)
    for call in (lambda: em.emitter_threshold(probes), lambda: em.label_emitters(probes, 1.0),
                 lambda: em.emitter_stats(probes, torch.zeros(2, 8, 16, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)),
                 lambda: em.emitters_from_probes(probes, np.zeros((2, 3))),
                 lambda: em.residual_probes(probes, torch.zeros(2, 8, 16, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
    for bad in (torch.rand(3, 8, 16), torch.rand(2, 4, 8, 16), torch.rand(2, 3, 1, 16), torch.rand(2, 3, 8, 1), torch.rand(0, 3, 8, 16),
                np.zeros((2, 3, 8, 16), np.float32)):
        with pytest.raises(ValueError):
            em.emitter_threshold(bad)
        with pytest.raises(ValueError):
            em.label_emitters(bad, 1.0)
    for ratio in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ratio"):
            em.emitter_threshold(probes, ratio)
    with pytest.raises(ValueError, match="min_solid_angle"):
        em.emitters_from_probes(probes, np.zeros((2, 3)), min_solid_angle=-1.0)
    with pytest.raises(ValueError, match="max_emitters"):
        em.emitters_from_probes(probes, np.zeros((2, 3)), max_emitters=1.5)
    with pytest.raises(ValueError, match="size"):
        em.extract_emitters(None, torch.zeros(1, 3), size=64)
