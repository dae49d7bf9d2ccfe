"""pn_bvh_walk.h under its three users at once: one MeshBVH is handed as accel to trace_mesh, closest_point and
winding_number in turn, on trees of one, two and three faces and on the complete tree of the `stack` mesh, with 65 query rows
(one wave and one lane).  The ordered walk's two users equal brute force bit for bit, under the conditions test_gpu_bvh.py
and test_gpu_meshdist.py state for that equality (the numpy restatements count no pair the candidate rule loses; on `stack`,
whose faces have no area, the tracer is held to the restatement and to brute force on the rays that lose none); the
pre-order walk equals the numpy restatement on the device tree within test_gpu_winding.py's derived tolerance; and the three
queries leave the tree's rows as they found them, byte for byte."""
import numpy as np
import pytest
import torch

import _meshdist_ref as md
import _winding_ref as ref
from _gpu_mesh import N, T, bits_equal, check_w

pytestmark = pytest.mark.gpu
ROWS = 65
MESHES = {"F = 1": "ico3[:1]", "F = 2": "ico3[:2]", "F = 3": "ico3[:3]", "ico3[:3]": "ico3[:3]", "stack": "stack"}


def queries(name):
    """65 of the mesh's query points (on vertices, edges and faces, in the box, far away, the NaN row and the inf row last),
    and 65 finite rays: from test_bvh_cpu.py's EYE at the 63 finite points, and from two of them back at the eye"""
    bspec = md.bvh_spec()
    pts = md.query_points(name)[np.r_[np.linspace(0, 997, ROWS - 2).astype(np.int64), 998, 999]]
    eye = np.broadcast_to(np.asarray(bspec.EYE, np.float32), (ROWS - 2, 3))
    o = np.concatenate([eye, pts[:2]]).astype(np.float32)
    d = np.concatenate([pts[:ROWS - 2] - eye, eye[:2] - pts[:2]]).astype(np.float32)
    return pts, o, d


def words(x):
    return np.ascontiguousarray(x).view(np.int32)


@pytest.mark.parametrize("case", sorted(MESHES))
def test_one_tree_under_the_three_walks(case):
    from pano_nerf_amd import meshdist, objects, winding
    name = MESHES[case]
    bspec = md.bvh_spec()
    v, f = md.meshes()[name]
    if case.startswith("F = "):  # test_gpu_bvh.py's own one, two and three faces: the same sphere
        sv, sf = bspec.spec.icosphere(3, bspec.RADIUS, bspec.CENTRE)
        assert np.array_equal(sv, v) and np.array_equal(sf[:len(f)], f)
    pts, o, d = queries(name)
    assert len(pts) == len(o) == ROWS and np.isfinite(o).all() and np.isfinite(d).all() and not np.isfinite(pts[-2:]).all(1).any()
    tp, to, td, tv, tf = T(pts), T(o), T(d), T(v), T(f, torch.int32)
    tree = objects.MeshBVH.build(tv, tf)
    before = N(tree.nodes).tobytes()

    # rays: the walk is the contract's restatement, and brute force on every ray of which the candidate rule loses no pair
    # (the faces of `stack` have no area: what the ray / triangle test accepts of them there is mostly no candidate)
    rt, rface, rbary, lost, accepted = bspec.candidate_trace(o, d, v, f)
    tm = np.where(np.arange(ROWS) % 2 == 0, rt, rt * np.float32(2)).astype(np.float32)  # exclusive: every other winner is cut
    tm[~np.isfinite(tm)] = 1.0
    for t_max, want in ((None, (rt, rface, rbary)), (tm, bspec.candidate_trace(o, d, v, f, t_max=tm)[:3])):
        tt = None if t_max is None else T(t_max)
        got = [N(x) for x in objects.trace_mesh(to, td, tv, tf, t_max=tt, accel=tree)]
        assert all(np.array_equal(words(a), words(b)) for a, b in zip(got, want))
        brute = [N(x) for x in objects.trace_mesh(to, td, tv, tf, t_max=tt)]
        differ = [r for r in range(ROWS) if any(not np.array_equal(words(a[r]), words(b[r])) for a, b in zip(got, brute))]
        print(f"{case}, t_max {t_max is not None}: {int((got[1] >= 0).sum())} hits, {accepted} accepted pairs, {lost} lost, "
              f"{len(differ)} rays differ from brute force")
        for r in differ:
            assert bspec.candidate_trace(o[r:r + 1], d[r:r + 1], v, f, None if t_max is None else t_max[r:r + 1])[3] > 0, r
        assert np.array_equal(N(objects.trace_mesh(to, td, tv, tf, t_max=tt, any_hit=True, accel=tree)), want[1] >= 0)
    assert lost == 0 or name == "stack"

    # points: no violation of the candidate rule, so the walk is brute force
    answer = md.closest_point(pts, v, f)
    assert answer["violations"] == 0
    got = meshdist.closest_point(tp, tv, tf, accel=tree)
    want = meshdist.closest_point(tp, tv, tf, accel=None)
    assert all(bits_equal(a, b) for a, b in zip(got, want)) and np.array_equal(N(got[1]), answer["face"])
    reach = float(np.median(answer["distance"][np.isfinite(answer["distance"])]))
    assert md.closest_point(pts, v, f, reach)["violations"] == 0
    got = meshdist.closest_point(tp, tv, tf, max_distance=reach, accel=tree)
    assert all(bits_equal(a, b) for a, b in zip(got, meshdist.closest_point(tp, tv, tf, max_distance=reach, accel=None)))

    # winding: the pre-order walk on the shared stack and row reader is the restatement on the device tree
    for beta in (2.0, 1e6):
        w = winding.winding_number(tp, tv, tf, accel=tree, beta=beta)
        rw = ref.walk(pts, v, f, N(tree.nodes), N(tree._winding_moments), beta)
        assert rw["visits"].max() <= 2 * len(f) - 1
        check_w(w, rw, rw["visits"], f"{case} walk, beta {beta:g}")

    assert N(tree.nodes).tobytes() == before
