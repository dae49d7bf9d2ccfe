"""The numpy restatement of the mesh operations (tests/_meshops_ref.py) held to facts that do not depend on it: planes stay
planes, cube corners stay corners within a bound computed here, spheres stay closed, the result does not depend on the
summation order beyond 1e-12 cell, almost no cluster sits on a discrete decision, and the components of the flood fill
are what the meshes were built to have.  No GPU: this is what makes one fp32 ulp the right tolerance for the GPU tests."""
import importlib

import numpy as np
import pytest

import _meshops_ref as ref


@pytest.fixture(scope="module")
def results():
    out = {}
    for name, cell in ref.SIMPLIFY_CASES:
        v, f, origin = ref.simplify_case(name)
        out[name, cell] = (v, f, ref.simplify(v, f, cell, origin))
    return out


def sym(a6):
    return np.array([[a6[0], a6[1], a6[2]], [a6[1], a6[3], a6[4]], [a6[2], a6[4], a6[5]]])


def test_plane_stays_a_plane(results):
    """64 x 64 quads on z = x / 2 + y / 4 (dyadic coordinates: the fp32 vertices lie on it exactly): every output vertex
    lies on the plane to 1e-12 x extent, whether it was solved or fell back to the mean"""
    v, f, r = results["plane", 0.3]
    n = np.array([0.5, 0.25, -1.0])
    dist = np.abs(r["vertices"] @ n) / np.linalg.norm(n)
    extent = float(np.linalg.norm(v.max(0) - v.min(0)))
    print(f"plane: {len(r['vertices'])} vertices, worst distance {dist.max():.3e} (bound {1e-12 * extent:.3e})")
    assert len(r["faces"]) > 50 and dist.max() <= 1e-12 * extent
    assert ref.edge_counts(r["faces"])["nonmanifold"] == 0 and ref.edge_counts(r["faces"])["inconsistent"] == 0


@pytest.mark.parametrize("cell", [0.25, 0.3, 0.5])
def test_cube_corners_stay_corners(results, cell):
    """The cluster that holds a corner of [-1, 1]^3 sees three orthogonal families of planes, so A has full rank and the
    minimiser of the quadric alone is the corner p: A p = -b.  The regularised solution obeys x - p = (A + s I)^-1 s (xbar - p)
    with s = lam t, hence |x - p| <= s / lambda_min(A) |xbar - p|: the bound is computed here from the restatement's A, t and
    xbar.  Placing the vertex at the mean instead misses the corner by at least 10 x as much."""
    v, f, r = results["cube", cell]
    assert r["flags_all"].max() == 0 and r["duplicates"] == 0
    assert ref.euler(len(r["vertices"]), r["faces"]) == 2
    assert ref.edge_counts(r["faces"]) == {"boundary": 0, "nonmanifold": 0, "inconsistent": 0}
    assert len(np.unique(np.sort(r["faces"], 1), axis=0)) == len(r["faces"])
    corners = np.nonzero((np.abs(v) == 1.0).all(1))[0]
    assert len(corners) == 8
    worst = 0.0
    for i in corners:
        k = r["rank"][i]
        p = v[i].astype(np.float64)
        lam_min = np.linalg.eigvalsh(sym(r["A"][k]))[0]
        assert lam_min > 0
        mean = r["centres"][k] + r["xbar"][k]
        got = r["centres"][k] + r["x"][k]
        bound = 1e-3 * r["t"][k] / lam_min * np.linalg.norm(mean - p)
        err = np.linalg.norm(got - p)
        worst = max(worst, err)
        assert err <= bound + 1e-12, (cell, i, err, bound)
        assert np.linalg.norm(mean - p) >= 10.0 * err
    # the worst distance of any output vertex to the cube's surface
    q = np.abs(r["vertices"])
    surf = np.abs(q.max(1) - 1.0)
    print(f"cube cell {cell}: worst corner error {worst:.3e}, worst surface error {surf.max():.3e}")
    assert surf.max() <= 1e-3


@pytest.mark.parametrize("cell", [0.25, 0.3, 0.5])
def test_icosphere(results, cell):
    """5120 faces, origin 0.01 below the minimum.  At 0.25 and 0.5 the result is a closed manifold of Euler characteristic
    2 without a fallback; at 0.3 three clusters fall back to their mean and three duplicate faces go: the case that
    exercises both rules (its edge census says what that did to the topology).  Every output vertex lies in the box of its
    cell, hence within sqrt(3) cell of an input vertex."""
    v, f, r = results["ico", cell]
    census = ref.edge_counts(r["faces"])
    fell, dups = int((r["flags_all"] == 1).sum()), r["duplicates"]
    print(f"icosphere cell {cell}: {len(r['faces'])} faces, {fell} fallbacks, {dups} duplicates, {census}")
    assert ref.euler(len(r["vertices"]), r["faces"]) == 2
    if cell == 0.3:
        assert fell == 3 and dups == 3
    else:
        assert fell == 0 and dups == 0 and census == {"boundary": 0, "nonmanifold": 0, "inconsistent": 0}
    half = 0.5 * r["cell"]
    inside = np.abs(r["vertices"] - r["centres"][r["used"]])
    assert inside.max() <= half * (1 + 1e-12)
    d = np.sqrt(((r["vertices"][:, None, :] - v.astype(np.float64)[None]) ** 2).sum(-1)).min(1)
    assert d.max() <= np.sqrt(3.0) * r["cell"]
    assert np.array_equal(np.unique(r["faces"]), np.arange(len(r["vertices"])))  # exactly the clusters a face uses


def test_order_independence(results):
    """Permuting the order of every sum within every cluster moves the solution by less than 1e-12 cell (the condition
    number is about 1 / lam = 1000): an implementation that follows the stated order is therefore far inside one fp32 ulp"""
    worst = 0.0
    for (name, cell), (v, f, r) in results.items():
        origin = ref.simplify_case(name)[2]
        for seed in (0, 1):
            p = ref.simplify(v, f, cell, origin, order=np.random.RandomState(seed))
            assert np.array_equal(p["flags_all"], r["flags_all"]) and np.array_equal(p["faces"], r["faces"])
            worst = max(worst, float(np.abs(p["x"] - r["x"]).max() / r["cell"]))
    print(f"order independence: worst move {worst:.3e} cell")
    assert worst < 1e-12


def test_fragile_cap(results):
    """at most 1 % of the clusters of any shared mesh sit on a discrete decision (here: none; the nearest is printed)"""
    for (name, cell), (v, f, r) in results.items():
        frac = r["fragile_all"].mean()
        near = (r["margin"][r["t"] != 0] / r["cell"]).min()
        print(f"{name} cell {cell}: {int(r['fragile_all'].sum())} fragile of {r['K']}, nearest decision {near:.2e} cell")
        assert frac <= 0.01


def test_attribute_means(results):
    """normals and colours of a cluster are the means of its vertices' rows, the normals renormalised"""
    v, f, origin = ref.simplify_case("ico")
    nrm, col = ref.attributes(v)
    r = ref.simplify(v, f, 0.5, origin, normals=nrm, colors=col)
    k = int(np.argmax(np.bincount(r["rank"])))
    members = r["rank"] == k
    want_c = col[members].astype(np.float64).mean(0)
    want_n = nrm[members].astype(np.float64).mean(0)
    want_n /= np.linalg.norm(want_n)
    j = np.cumsum(r["used"])[k] - 1
    assert np.allclose(r["colors"][j], want_c, rtol=0, atol=1e-14) and np.allclose(r["normals"][j], want_n, rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------------------ components
EXPECTED = {"spheres_floater": (3, [320, 80, 4]), "fans": (1, [12]), "strip": (1, [4096]), "strip_long": (1, [9000]), "serpentine": (1, None),
            "unreferenced": (1, [12]), "triangle": (1, [1]), "empty": (0, [])}


@pytest.mark.parametrize("name", list(EXPECTED))
def test_components(name):
    v, f = ref.component_cases()[name]
    vlab, flab, C = ref.components(f, len(v))
    count, faces = EXPECTED[name]
    assert C == count
    st = ref.component_stats(v, f, flab, vlab, C)
    if faces is not None:
        assert st["faces"].tolist() == faces
    assert st["faces"].sum() == len(f) and st["vertices"].sum() == int((vlab >= 0).sum())
    # labels ascend with the smallest vertex index of the component
    firsts = [int(np.nonzero(vlab == c)[0][0]) for c in range(C)]
    assert firsts == sorted(firsts)
    if name == "unreferenced":
        assert vlab[0] == -1 and (vlab[-2:] == -1).all() and (vlab[1:-2] == 0).all()
    if name == "spheres_floater":  # closed and wound outwards: area and volume of the polyhedra, near the spheres'
        assert abs(st["area"][0] - 4 * np.pi) < 0.3 and abs(st["volume"][0] - 4 * np.pi / 3) < 0.2
        assert abs(st["volume"][2] - 0.25 ** 3 / 6) < 1e-12
        assert np.allclose(st["bbox"][2], [5, 5, 5, 5.25, 5.25, 5.25])


def test_filter_components():
    v, f = ref.component_cases()["spheres_floater"]
    (nv, nf, _, _), vmap, fmap = ref.filter_components(v, f, min_faces=5)
    assert len(nf) == 400 and len(nv) == len(v) - 4 and (vmap[-4:] == -1).all() and np.array_equal(fmap, np.arange(400))
    assert np.array_equal(nv[nf], v[f[fmap]])  # the same triangles
    (nv, nf, _, _), vmap, fmap = ref.filter_components(v, f, keep_largest=1)
    assert len(nf) == 320 and np.array_equal(nv, v[:len(nv)])
    (nv, nf, _, _), _, _ = ref.filter_components(v, f, keep_largest=2, by="faces", min_area=1.0)
    assert len(nf) == 400
    # a tie goes to the lower label: two equal spheres
    a = ref.icosphere(1, 1.0)
    v2, f2 = ref.join(a, (a[0] + np.float32(4.0), a[1]))
    (_, nf, _, _), _, fmap = ref.filter_components(v2, f2, keep_largest=1, by="faces")
    assert np.array_equal(fmap, np.arange(len(a[1])))


def test_edge_counts():
    v, f = ref.cube(2)
    assert ref.edge_counts(f) == {"boundary": 0, "nonmanifold": 0, "inconsistent": 0}
    assert ref.edge_counts(f[1:])["boundary"] == 3
    flipped = f.copy()
    flipped[0] = flipped[0, ::-1]
    assert ref.edge_counts(flipped)["inconsistent"] == 3
    assert ref.edge_counts(np.concatenate([f, [[f[0, 0], f[0, 1], 25]]]))["nonmanifold"] == 1


def test_symbols_are_declared():
    lib = importlib.import_module("pano_nerf_amd._lib")
    for name in ("pn_mesh_check", "pn_mesh_components", "pn_mesh_labels", "pn_mesh_component_stats", "pn_cluster_keys",
                 "pn_cluster_faces", "pn_cluster_solve"):
        assert name in lib.SIGNATURES, name
    meshops = importlib.import_module("pano_nerf_amd.meshops")
    pkg = importlib.import_module("pano_nerf_amd")
    assert pkg.meshops is meshops and pkg.simplify_mesh is meshops.simplify_mesh
