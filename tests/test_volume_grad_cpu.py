"""The numpy restatement of the marcher's reverse sweep (tests/_volume_grad_ref.py) against what it must equal: the forward
restatement, central differences in fp64, closed forms of a homogeneous slab, and itself under a permutation of the rows.
No GPU."""
import functools

import numpy as np

import _volume_grad_ref as gref
import _volume_ref as ref
import _volume_scenes as scenes

H = 1e-6  # the difference step


def scene(name):
    data, bounds, deg, _ = scenes.volume(name)
    lo, step = scenes.placement(bounds, data.shape[:3])
    return data, lo, step, deg, scenes.march_step(bounds, data.shape[:3])


@functools.lru_cache(maxsize=None)
def upstream(seed=3):
    rng = np.random.default_rng(seed)
    R = scenes.rays()["origins"].shape[0]
    return rng.standard_normal((R, 3)).astype(np.float32), rng.standard_normal(R).astype(np.float32)


def ray_args():
    r = scenes.rays()
    return r["origins"], r["directions"], r["near"], r["far"]


def test_forward_sums_reproduce_the_forward_restatement():
    g, ga = upstream()
    for name in sorted(scenes.VOLUMES):
        data, lo, step, deg, ms = scene(name)
        for t_min in (0.0, 1e-3):
            want = ref.march(data, lo, step, deg, *ray_args(), ms, t_min)
            got = gref.march_grad(data, lo, step, deg, *ray_args(), ms, t_min, g, ga)
            # the same operations in the same order: the same fp64 values
            assert np.array_equal(got["rgb"], want["rgb"]) and np.array_equal(got["acc"], want["acc"]), name
            assert np.array_equal(got["marched"], want["marched"]) and np.array_equal(got["fragile"], want["fragile"])
            # U sums the same terms sample by sample instead of channel by channel: fp64 round-off of that sum apart
            dot = (g.astype(np.float64) * want["rgb"]).sum(1) + ga.astype(np.float64) * want["acc"]
            bound = 16 * 2.0 ** -52 * got["abs_u"]
            assert (np.abs(got["U"] - dot) <= bound).all(), (name, t_min, float(np.abs(got["U"] - dot).max()))
            assert not got["grad"][:, :][~np.isfinite(got["grad"])].size, name


def check_differences(name, entries):
    """central differences of L = sum_r g . rgb + g_acc acc in fp64 at the entries (vertex, channel) given"""
    data, lo, step, deg, ms = scene(name)
    g, ga = upstream()
    args = (lo, step, deg, *ray_args(), ms, 0.0)
    base = data.astype(np.float64)
    got = gref.march_grad(base, *args, g, ga, exact=True)
    N, Cg = got["grad"].shape
    flat = base.reshape(N, -1)
    # the round-off of the quotient: each L is a sum of terms of total magnitude sum_r (|g| . abs_rgb + |g_acc| acc)
    bound = 16 * 2.0 ** -52 * float(got["abs_u"].sum()) / H
    gated = gref.near_gate(base, *args, 10 * H)
    tested = left_out = 0
    worst = 0.0
    for v, ch in entries:
        tested += 1
        if gated[v]:
            left_out += 1
            continue
        L = []
        for sign in (1.0, -1.0):
            moved = flat.copy()
            moved[v, ch] += sign * H
            f = gref.forward(gref.Sweep(moved.reshape(base.shape), *args, exact=True), g, ga)
            L.append(float(f["U"].sum()))
        quotient = (L[0] - L[1]) / (2 * H)
        err = abs(quotient - got["grad"][v, ch])
        worst = max(worst, err)
        assert err <= bound, (name, v, ch, quotient, got["grad"][v, ch], bound)
    assert left_out <= 0.1 * tested, (name, left_out, tested)
    print(f"{name}: {tested - left_out} entries, worst difference {worst:.3e} (bound {bound:.3e}), {left_out} near a gate")
    return got


def test_central_differences_one_cell():
    check_differences("one_cell", [(v, ch) for v in range(8) for ch in range(4)])  # every entry there is


def test_central_differences_strides():
    rng = np.random.default_rng(17)
    data = scenes.volume("strides")[0]
    N, Cg = data.shape[0] * data.shape[1] * data.shape[2], 13
    picks = rng.choice(N * Cg, 32, replace=False)
    got = check_differences("strides", [(int(p // Cg), int(p % Cg)) for p in picks])
    assert got["grad"].shape == (N, Cg)  # the attribute channels get no gradient: they are not even there


def test_homogeneous_slab_closed_forms():
    res, s, colour = (4, 5, 3), 1.7, np.array([0.9, 0.5, 0.2])
    data = np.zeros(res + (4,), np.float32)
    data[..., 0] = s
    data[..., 1:] = colour
    lo, step = scenes.placement(scenes.BOUNDS, res)
    ms = scenes.march_step(scenes.BOUNDS, res)
    # rays that start and end inside the box: every lattice point composites
    o = np.array([[0.0, 0.0, 0.0], [-0.3, 0.2, -0.4], [0.4, -0.2, 0.3]], np.float32)
    d = np.array([[0.3, 0.2, -0.4], [2.0, 0.5, 1.0], [-1.0, 0.0, 0.0]], np.float32)
    near, far = np.array([0.0, 0.05, 0.1], np.float32), np.array([0.9, 0.2, 0.6], np.float32)
    rng = np.random.default_rng(2)
    for r in range(3):
        g, ga = rng.standard_normal((1, 3)).astype(np.float32), rng.standard_normal(1).astype(np.float32)
        got = gref.march_grad(data, lo, step, 0, o[r:r + 1], d[r:r + 1], near[r:r + 1], far[r:r + 1], ms, 0.0, g, ga)
        sw = gref.Sweep(data, lo, step, 0, o[r:r + 1], d[r:r + 1], near[r:r + 1], far[r:r + 1], ms, 0.0)
        n, stepw = int(sw.n[0]), float(sw.stepw[0])
        assert n >= 3 and got["count"][:, 0].sum() == 8 * n  # all n samples composite
        s64 = float(np.float32(s))
        col = ref.SH_C[0] * data[0, 0, 0, 1:].astype(np.float64)
        gu = float((g[0].astype(np.float64) * col).sum() + float(ga[0]))
        want = stepw * n * np.exp(-s64 * stepw * n) * gu  # the corner weights of a sample sum to 1
        scale = stepw * n * abs(gu)
        assert abs(got["grad"][:, 0].sum() - want) <= 1e-12 * scale, (r, got["grad"][:, 0].sum(), want)
        acc = 1.0 - np.exp(-s64 * stepw * n)
        assert abs(got["acc"][0] - acc) <= 1e-13
        for ch in range(3):
            want_c = ref.SH_C[0] * acc * float(g[0, ch])
            assert abs(got["grad"][:, 1 + ch].sum() - want_c) <= 1e-12 * abs(float(g[0, ch])), (r, ch)


def test_quantised_sums_do_not_depend_on_the_order_of_the_rows():
    g, ga = upstream()
    for name in ("strides", "nan"):
        data, lo, step, deg, ms = scene(name)
        o, d, tn, tf = ray_args()
        one = gref.march_grad(data, lo, step, deg, o, d, tn, tf, ms, 1e-3, g, ga, quantum=gref.QUANTUM)
        p = np.random.default_rng(8).permutation(o.shape[0])
        two = gref.march_grad(data, lo, step, deg, o[p], d[p], tn[p], tf[p], ms, 1e-3, g[p], ga[p], quantum=gref.QUANTUM)
        assert not one["flag"] and not two["flag"] and one["sums"].any()
        assert np.array_equal(one["sums"], two["sums"]), name
        # and they are the fp64 gradient to half a quantum per contribution
        assert (np.abs(one["sums"] * gref.QUANTUM - one["grad"]) <= 0.5 * gref.QUANTUM * one["count"] + 1e-18).all()


def test_quantise_flags_what_it_cannot_hold():
    m, bad = gref.quantise(np.array([0.5, 1.5, 2.5, -0.5, np.nan, np.inf, 2.0 ** 52, 2.0 ** 52 - 1]), 1.0)
    assert m.tolist() == [0, 2, 2, 0, 0, 0, 0, 2 ** 52 - 1] and bad.tolist() == [False] * 4 + [True] * 3 + [False]
