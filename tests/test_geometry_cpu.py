"""Geometry export without a GPU: a numpy restatement of the marching-tetrahedra contract of include/panonerf_hip.h (the
executable spec the kernels are compared against in test_gpu_geometry.py), checked here on closed surfaces; the PLY
writer against a minimal reader; and the argument checks that run before any launch."""
import os

import numpy as np
import pytest
import torch

import pano_nerf_amd as pn
from pano_nerf_amd import geometry

# ------------------------------------------------------------------------------------------------ the spec
OFFSETS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]])
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]  # xyz, xzy, yxz, yzx, zxy, zyx
TET_EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def tet_vertices(perm):
    """T0 = p, T1 = p + e_a, T2 = p + e_a + e_b, T3 = p + (1, 1, 1) as corner offsets [4, 3]"""
    a, b, _ = perm
    t = np.zeros((4, 3), dtype=np.int64)
    t[1, a] = 1
    t[2, a] = t[2, b] = 1
    t[3] = 1
    return t


def case_table():
    """case -> triangles (tetrahedron-edge triples) for a positively oriented tetrahedron, derived from the rule: a lone
    vertex gives its three edges in ascending order; two and two (inside a < b, outside c < d) give (ac, ad, bd),
    (ac, bd, bc); each wound so that its normal points from the inside vertices to the outside ones."""
    tv = tet_vertices(PERMS[0]).astype(np.float64)
    edge = lambda u, w: TET_EDGES.index((min(u, w), max(u, w)))
    table = []
    for case in range(16):
        ins = [q for q in range(4) if case >> q & 1]
        outs = [q for q in range(4) if not case >> q & 1]
        tris = []
        if len(ins) in (1, 3):
            a = ins[0] if len(ins) == 1 else outs[0]
            rest = [q for q in range(4) if q != a]
            tris.append([edge(a, r) for r in rest])
        elif len(ins) == 2:
            (a, b), (c, d) = ins, outs
            tris += [[edge(a, c), edge(a, d), edge(b, d)], [edge(a, c), edge(b, d), edge(b, c)]]
        out = []
        for t in tris:
            m = [tv[list(TET_EDGES[e])].mean(0) for e in t]
            n = np.cross(m[1] - m[0], m[2] - m[0])
            if np.dot(n, tv[outs].mean(0) - tv[ins].mean(0)) < 0:
                t = [t[0], t[2], t[1]]
            out.append(t)
        table.append(out)
    return table


CASES = case_table()


def placement(res, bounds):
    if bounds is None:
        return np.zeros(3, np.float32), np.ones(3, np.float32)
    lo, hi = np.asarray(bounds[0], np.float64), np.asarray(bounds[1], np.float64)
    return lo.astype(np.float32), ((hi - lo) / (np.asarray(res) - 1)).astype(np.float32)


def mt_reference(sigma, level, bounds=None):
    """(vertices [V, 3] fp32, faces [F, 3] int32) exactly as the contract orders them; also returns the edge ids."""
    s = np.ascontiguousarray(sigma, dtype=np.float32)
    nx, ny, nz = s.shape
    level = np.float32(level)
    lo, step = placement(s.shape, bounds)
    inside = s > level
    vid = np.arange(s.size, dtype=np.int64).reshape(s.shape)
    ijk = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1)
    eids, pts = [], []
    for si, o in enumerate(OFFSETS):
        lw = (slice(0, nx - o[0]), slice(0, ny - o[1]), slice(0, nz - o[2]))
        up = (slice(o[0], nx), slice(o[1], ny), slice(o[2], nz))
        cross = inside[lw] != inside[up]
        sa, sb = s[lw][cross], s[up][cross]
        t = ((level - sa) / (sb - sa)).astype(np.float32)
        ia = ijk[lw][cross]
        pa = lo + ia.astype(np.float32) * step
        pb = lo + (ia + o).astype(np.float32) * step
        pts.append((pa + t[:, None] * (pb - pa)).astype(np.float32))
        eids.append(vid[lw][cross] * 7 + si)
    eid = np.concatenate(eids)
    order = np.argsort(eid, kind="stable")
    eid_sorted = eid[order]
    verts = np.concatenate(pts)[order] if len(eid) else np.zeros((0, 3), np.float32)
    # faces: key (cell, tetrahedron, triangle)
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    cell_ijk = ijk[:cx, :cy, :cz].reshape(-1, 3)
    keys, tris = [], []
    for ti, perm in enumerate(PERMS):
        tv = tet_vertices(perm)
        case = np.zeros(len(cell_ijk), np.int64)
        for q in range(4):
            c = cell_ijk + tv[q]
            case |= inside[c[:, 0], c[:, 1], c[:, 2]].astype(np.int64) << q
        for slot in range(2):
            for cs in range(16):
                if slot >= len(CASES[cs]):
                    continue
                sel = np.nonzero(case == cs)[0]
                if not len(sel):
                    continue
                idx = []
                for e in CASES[cs][slot]:
                    lo_v, hi_v = tv[TET_EDGES[e][0]], tv[TET_EDGES[e][1]]
                    off = hi_v - lo_v
                    si = int(np.nonzero((OFFSETS == off).all(1))[0][0])
                    u = cell_ijk[sel] + lo_v
                    ids = vid[u[:, 0], u[:, 1], u[:, 2]] * 7 + si
                    idx.append(np.searchsorted(eid_sorted, ids))
                tri = np.stack(idx, 1)
                if np.linalg.det(np.stack([tv[1] - tv[0], tv[2] - tv[0], tv[3] - tv[0]])) < 0:
                    tri = tri[:, [0, 2, 1]]
                tris.append(tri)
                keys.append(sel * 12 + ti * 2 + slot)
    if tris:
        key = np.concatenate(keys)
        faces = np.concatenate(tris)[np.argsort(key, kind="stable")].astype(np.int32)
    else:
        faces = np.zeros((0, 3), np.int32)
    return verts, faces, eid_sorted


def grid_coords(res, bounds):
    lo, step = placement(res, bounds)
    axes = [lo[a] + np.arange(res[a]).astype(np.float32) * step[a] for a in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1)


def edge_stats(faces):
    """(undirected edge -> face count, directed edge count array) of a triangle list"""
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    und = np.sort(d, 1)
    _, und_count = np.unique(und[:, 0] * (1 << 32) + und[:, 1], return_counts=True)
    _, dir_count = np.unique(d[:, 0] * (1 << 32) + d[:, 1], return_counts=True)
    return und_count, dir_count


def euler(verts, faces):
    und_count, _ = edge_stats(faces)
    return len(verts) - len(und_count) + len(faces)


BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def sphere_field(res, r=0.6, center=(0.0, 0.0, 0.0)):
    x = grid_coords(res, BOX).astype(np.float64) - np.asarray(center)
    return (r - np.linalg.norm(x, axis=-1)).astype(np.float32)


def torus_field(res, big=0.55, small=0.25):
    x = grid_coords(res, BOX).astype(np.float64)
    q = np.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2) - big
    return (small - np.sqrt(q ** 2 + x[..., 2] ** 2)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ spec checks
def test_case_table_is_the_documented_one():
    want = {1: [[0, 1, 2]], 2: [[0, 4, 3]], 3: [[1, 2, 4], [1, 4, 3]], 4: [[1, 3, 5]], 5: [[0, 5, 2], [0, 3, 5]],
            6: [[0, 4, 5], [0, 5, 1]], 7: [[2, 4, 5]], 8: [[2, 5, 4]], 9: [[0, 1, 5], [0, 5, 4]],
            10: [[0, 5, 3], [0, 2, 5]], 11: [[1, 5, 3]], 12: [[1, 3, 4], [1, 4, 2]], 13: [[0, 3, 4]], 14: [[0, 2, 1]]}
    assert CASES[0] == [] and CASES[15] == []
    for c, tris in want.items():
        assert CASES[c] == tris, c
    # tetrahedron orientation: the sign of det(e_a, e_b, e_c) = the parity of the permutation
    signs = [round(np.linalg.det(np.stack([tet_vertices(p)[q] - tet_vertices(p)[0] for q in (1, 2, 3)]))) for p in PERMS]
    assert signs == [1, -1, -1, 1, 1, -1]


@pytest.mark.parametrize("res", [(20, 20, 20), (23, 17, 19)])
def test_sphere_is_a_closed_genus_0_surface(res):
    v, f, eid = mt_reference(sphere_field(res), 0.0, BOX)
    assert len(v) > 100 and len(f) > 100
    assert np.all(np.diff(eid) > 0)  # ascending, distinct edge ids
    assert euler(v, f) == 2
    und, dirc = edge_stats(f)
    assert np.all(und == 2)   # watertight: every undirected edge in exactly two faces
    assert np.all(dirc == 1)  # consistently oriented: every directed edge once
    a, b, c = v[f[:, 0]].astype(np.float64), v[f[:, 1]].astype(np.float64), v[f[:, 2]].astype(np.float64)
    n = np.cross(b - a, c - a)
    area = np.linalg.norm(n, axis=1)
    big = area > 1e-9 * area.max()
    assert np.all(np.einsum("ij,ij->i", n, (a + b + c) / 3)[big] > 0)  # outward: the outside is sigma <= level


def test_torus_has_euler_characteristic_0():
    v, f, _ = mt_reference(torus_field((40, 40, 24)), 0.0, BOX)
    assert euler(v, f) == 0
    und, dirc = edge_stats(f)
    assert np.all(und == 2) and np.all(dirc == 1)


def test_two_spheres_and_degenerate_fields():
    res = (21, 21, 21)
    s = np.maximum(sphere_field(res, 0.3, (-0.45, 0, 0)), sphere_field(res, 0.3, (0.45, 0, 0)))
    v, f, _ = mt_reference(s, 0.0, BOX)
    assert euler(v, f) == 4
    for field in (np.ones(res, np.float32), -np.ones(res, np.float32), np.zeros(res, np.float32)):
        v, f, _ = mt_reference(field, 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3)


def test_open_surface_boundary_edges_lie_on_the_box():
    # a sphere cut by the grid: edges used by one face run along the box boundary
    res = (17, 17, 17)
    v, f, _ = mt_reference(sphere_field(res, 0.9, (0.5, 0.0, 0.0)), 0.0, BOX)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    und = np.sort(d, 1)
    k, cnt = np.unique(und[:, 0] * (1 << 32) + und[:, 1], return_counts=True)
    assert cnt.max() == 2 and (cnt == 1).any()
    single = np.stack([k >> 32, k & 0xFFFFFFFF], 1)[cnt == 1]
    ends = v[single.reshape(-1)].reshape(-1, 2, 3)
    on = np.isclose(np.abs(ends), 1.0, atol=1e-6)
    assert np.all((on[:, 0] & on[:, 1]).any(-1))  # both endpoints on one common face of the box


# ------------------------------------------------------------------------------------------------ PLY
def read_ply(path):
    """Minimal binary little-endian PLY reader for the layout write_ply produces."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0" and head[-1] == "end_header"
    elems, cur = [], None
    for line in head[2:-1]:
        w = line.split()
        if w[0] == "element":
            cur = [w[1], int(w[2]), []]
            elems.append(cur)
        elif w[0] == "property":
            cur[2].append(tuple(w[1:]))
    (vn, nv, vprops), (fn, nf, fprops) = elems
    assert vn == "vertex" and fn == "face" and fprops == [("list", "uchar", "int", "vertex_indices")]
    kinds = {"float": "<f4", "uchar": "u1"}
    vdt = np.dtype([(p[1], kinds[p[0]]) for p in vprops])
    vrec = np.frombuffer(data, vdt, nv, end)
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    frec = np.frombuffer(data, fdt, nf, end + nv * vdt.itemsize)
    assert end + nv * vdt.itemsize + nf * fdt.itemsize == len(data)
    assert np.all(frec["n"] == 3)
    return [p[1] for p in vprops], vrec, frec["i"].copy()


def test_write_ply_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    v = rng.normal(size=(50, 3)).astype(np.float32)
    f = rng.integers(0, 50, size=(70, 3)).astype(np.int32)
    n = rng.normal(size=(50, 3)).astype(np.float32)
    c = np.concatenate([rng.uniform(-0.2, 1.2, size=(48, 3)), [[0.0, 0.5, 1.0], [1 / 255, 254.4 / 255, 254.6 / 255]]])
    p = str(tmp_path / "m.ply")
    geometry.write_ply(p, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n), torch.from_numpy(c).float())
    names, vrec, faces = read_ply(p)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert vrec.dtype.itemsize == 27
    np.testing.assert_array_equal(np.stack([vrec["x"], vrec["y"], vrec["z"]], 1), v)
    np.testing.assert_array_equal(np.stack([vrec["nx"], vrec["ny"], vrec["nz"]], 1), n)
    col = np.stack([vrec["red"], vrec["green"], vrec["blue"]], 1)
    np.testing.assert_array_equal(col, np.rint(np.clip(c.astype(np.float32), 0, 1) * 255).astype(np.uint8))
    assert col[-2].tolist() == [0, 128, 255] and col[-1].tolist() == [1, 254, 255]
    np.testing.assert_array_equal(faces, f)
    # positions only; empty faces
    geometry.write_ply(p, v, np.zeros((0, 3), np.int32))
    names, vrec, faces = read_ply(p)
    assert names == ["x", "y", "z"] and vrec.dtype.itemsize == 12 and faces.shape == (0, 3)
    with open(p, "rb") as fh:
        assert fh.read().startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 50\nproperty float x\n")


# ------------------------------------------------------------------------------------------------ validation
@pytest.fixture(scope="module")
def built():
    lib = pn._lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return lib.load()


def test_argument_checks_before_any_launch(built, tmp_path):
    s = torch.zeros(4, 5, 6)
    with pytest.raises(ValueError, match="nx, ny, nz"):
        geometry.marching_tetrahedra(torch.zeros(4, 5), 0.0)
    with pytest.raises(ValueError, match=">= 2"):
        geometry.marching_tetrahedra(torch.zeros(4, 1, 6), 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.marching_tetrahedra(s, 0.0)
    pano = pn.PanoMipNeRF(num_samples=8, rgb_activation="softplus", mlp_num_density_channels=5)
    mip = pn.MipNeRF(num_samples=8, rgb_activation="softplus")
    with pytest.raises(ValueError, match="albedo"):
        geometry.extract_mesh(mip, BOX, 8, 0.5, colors="albedo")
    with pytest.raises(ValueError, match="albedo"):
        geometry.query_field(mip, torch.zeros(3, 3), outputs=("albedo",))
    with pytest.raises(ValueError, match="colors"):
        geometry.extract_mesh(pano, BOX, 8, 0.5, colors="bogus")
    with pytest.raises(ValueError, match=r"\[M, 3\]"):
        geometry.query_field(pano, torch.zeros(3, 3, 1))
    with pytest.raises(ValueError, match="viewdirs"):
        geometry.query_field(pano, torch.zeros(3, 3), outputs=("rgb",))
    with pytest.raises(ValueError, match="unknown"):
        geometry.query_field(pano, torch.zeros(3, 3), outputs=("density",))
    with pytest.raises(ValueError, match="resolution"):
        geometry.density_grid(pano, BOX, 1)
    with pytest.raises(ValueError, match="resolution"):
        geometry.density_grid(pano, BOX, (4, 4))
    with pytest.raises(ValueError, match="bounds"):
        geometry.density_grid(pano, ((0, 0), (1, 1)), 4)
    for call in (lambda: geometry.query_field(pano, torch.zeros(3, 3)),
                 lambda: geometry.density_grid(pano, BOX, 4),
                 lambda: geometry.extract_mesh(pano, BOX, 4, 0.5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="vertices"):
        geometry.write_ply(str(tmp_path / "x.ply"), np.zeros((3, 2)), np.zeros((1, 3), np.int32))
    with pytest.raises(ValueError, match="colors"):
        geometry.write_ply(str(tmp_path / "x.ply"), np.zeros((3, 3)), np.zeros((1, 3), np.int32), colors=np.zeros((2, 3)))
    assert pn.extract_mesh is geometry.extract_mesh


def test_library_shape_checks(built):
    # host-side status codes of the new entry points (nothing is launched: every call is refused before a launch)
    assert built.pn_mt_work_bytes(1, 4, 4) == -1
    assert built.pn_mt_work_bytes(1 << 11, 1 << 10, 1 << 10) == -1  # 2^31 vertices
    assert built.pn_mt_work_bytes(2, 2, 2) > 0
    assert built.pn_mt_count(4, 4, 1, None, 0.0, None, None, None) == -1
    assert built.pn_mt_count(4, 4, 4, None, 0.0, None, None, None) == -3
    assert built.pn_mt_emit(4, 4, 4, None, 0.0, None, 1 << 31, 0, 0, 0, 0, 1, 1, 1, None, None, None) == -1
    assert built.pn_grid_points(4, 4, 4, 60, 5, 0, 0, 0, 1, 1, 1, 0, None, None, None) == -1
    assert built.pn_grid_points(4, 4, 4, 0, 0, 0, 0, 0, 1, 1, 1, 0, None, None, None) == 0
    assert built.pn_field_epilogue(4, 1, -1.0, 0.0, None, None, None, None, 1, None, None, None) == -2
    assert built.pn_field_epilogue(4, 5, -1.0, 0.0, None, None, None, None, None, None, 1, None) == -3
