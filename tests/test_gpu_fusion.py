"""TSDF fusion on the GPU: pn_tsdf_integrate against the fp64 restatement of tests/_fusion_ref.py in the analytic room of
_relight_ref, its edge inputs, incremental integration, determinism, the mesh of a fused sphere against a derived bound, and
the composition of fuse_views / fused_mesh from render_view and query_field on a small random-initialised model.

Tolerance (from the number formats).  Both sides evaluate the header's formulas in fp64 on the same fp32 inputs and round
once; +, -, *, / and sqrt are correctly rounded on both, so away from the discrete decisions the restatement marks fragile
(at most 1 % of a scene's voxels, capped in test_fusion_cpu.py) the two fp64 results can differ only through atan2 / hypot,
which choose a pixel and enter no value: tsdf and weight are held to ONE fp32 ulp of the reference, and weight == 0 (the
voxels no view saw) has to agree exactly.  Each comparison prints the worst ulp distance it saw.

One launch takes every view of a call (the view loop runs inside the kernel), so there is no view-chunk boundary to test;
several views in one call are compared with the reference for that same single call in the parity tests (S = 3)."""
import functools

import numpy as np
import pytest
import torch

import _fusion_ref as ref

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


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def volume(res, bounds, trunc=ref.TRUNC):
    from pano_nerf_amd import fusion
    vol = fusion.TSDFVolume(bounds, res, trunc, device=dev())
    assert (vol.lo, vol.step) == ref.placement(bounds, res)
    return vol


def check(vol, want, what):
    """tsdf and weight of the device volume against the restatement's dict, on its non-fragile voxels; -> worst ulp"""
    ok = ~want["fragile"]
    got_t, got_w = N(vol.tsdf).astype(np.float64), N(vol.weight).astype(np.float64)
    assert np.array_equal((got_w == 0)[ok], (want["weight"] == 0)[ok]), what
    worst = 0.0
    for name, got, exp in (("tsdf", got_t, want["tsdf"]), ("weight", got_w, want["weight"])):
        d = (np.abs(got - exp) / ulp32(exp))[ok]
        worst = max(worst, float(d.max()))
        assert d.max() <= 1.0, (what, name, float(d.max()))
    print(f"{what}: worst {worst:.3f} ulp32 over {int(ok.sum())} voxels ({int((~ok).sum())} fragile, "
          f"{int((want['weight'] != 0).sum())} seen)")
    return worst


# ---------------------------------------------------------------------------------------------- 1. reference parity
@pytest.mark.parametrize("name,g,n", ref.PARITY, ids=[f"{c}-{g}-{n}" for c, g, n in ref.PARITY])
def test_reference_parity(name, g, n):
    """Worst distance seen on the first GPU run: 0.499 ulp32 (fisheye, room, 3 views), i.e. every value was the correctly
    rounded reference; the edge and incremental tests saw 0.474 and 0.493."""
    cam, c2ws, depth = ref.scene(name, n)
    res, bounds = ref.GRIDS[g]
    vol = volume(res, bounds)
    vol.integrate(T(depth), cam, c2ws)
    want = ref.integrate(res, vol.lo, vol.step, cam, c2ws, depth, trunc=vol.trunc)
    assert want["seen"].any()
    check(vol, want, f"{name}-{g}-{n}")
    assert np.array_equal(N(vol.observed()), N(vol.weight) > 0)


# -------------------------------------------------------------------------------------------------- 2. edge inputs
@pytest.mark.parametrize("name", ["pano", "pinhole"])
def test_edge_inputs(name):
    """NaN / 0 / negative / inf depths and depths above depth_max, zero and NaN confidences, a view of weight 0, a voxel
    exactly at a camera centre, voxels behind the pinhole, the panorama's seam, quarter meridians, poles and horizon facing
    grid voxels: all against the restatement.  Then a view with nothing valid in it leaves every bit of the volume alone."""
    cam, c2ws, depth, conf, vw, dmax, res, bounds = ref.edge_scene(name)
    vol = volume(res, bounds)
    vol.integrate(T(depth)[:, None], cam, c2ws, confidence=T(conf)[:, None], weights=vw, depth_max=dmax)
    want = ref.integrate(res, vol.lo, vol.step, cam, c2ws, depth, conf, vw, vol.trunc, dmax)
    assert want["seen"].any() and (~want["seen"]).any()
    check(vol, want, f"edge-{name}")
    # garbage where weight is 0 must survive too: the voxel keeps its bits
    junk = torch.where(vol.weight > 0, vol.tsdf, torch.full_like(vol.tsdf, 123.25))
    vol.tsdf.copy_(junk)
    t0, w0 = vol.tsdf.clone(), vol.weight.clone()
    for bad_depth, bad_conf, bad_w in ((np.full_like(depth[:1], np.nan), None, None), (depth[:1], np.zeros_like(conf[:1]), None),
                                       (depth[:1], None, [0.0]), (np.full_like(depth[:1], 2.0 * dmax), None, None)):
        vol.integrate(T(bad_depth), cam, c2ws[:1], confidence=None if bad_conf is None else T(bad_conf), weights=bad_w,
                      depth_max=dmax)
        assert bits_equal(vol.tsdf, t0) and bits_equal(vol.weight, w0)


# --------------------------------------------------------------------------------------------------- 3. incremental
@pytest.mark.parametrize("max_weight", [np.inf, 1.5])
@pytest.mark.parametrize("name", ["pano", "fisheye"])
def test_incremental(name, max_weight):
    """views A, then views B into the device's own result, against the restatement continuing that same fp32 volume"""
    cam, c2ws, depth = ref.scene(name, 3)
    res, bounds = ref.GRIDS["room"]
    vol = volume(res, bounds)
    vol.integrate(T(depth[:1]), cam, c2ws[:1], max_weight=max_weight)
    mid_t, mid_w = N(vol.tsdf), N(vol.weight)
    junk = np.where(mid_w > 0, mid_t, np.float32(-77.5))  # where weight is 0 the content of tsdf is ignored on input
    vol.tsdf.copy_(T(junk))
    vol.integrate(T(depth[1:]), cam, c2ws[1:], weights=[0.75, 2.0], max_weight=max_weight)
    want = ref.integrate(res, vol.lo, vol.step, cam, c2ws[1:], depth[1:], view_weights=[0.75, 2.0], trunc=vol.trunc,
                         max_weight=max_weight, tsdf=junk, weight=mid_w)
    both = (mid_w > 0) & want["seen"]
    assert both.any() and (want["seen"] & (mid_w == 0)).any()
    if np.isfinite(max_weight):
        assert (want["weight"] == max_weight).any() and (want["weight"] < max_weight)[want["weight"] > 0].any()
    check(vol, want, f"incremental-{name}-{max_weight}")


# -------------------------------------------------------------------------------------------- 5. the same bits again
def test_repeated_call_gives_the_same_bits():
    cam, c2ws, depth = ref.scene("cube", 3)
    res, bounds = ref.GRIDS["room"]
    out = []
    for _ in range(2):
        vol = volume(res, bounds)
        vol.integrate(T(depth), cam, c2ws, weights=[1.0, 0.5, 2.0])
        out.append((vol.tsdf.clone(), vol.weight.clone()))
    assert bits_equal(out[0][0], out[1][0]) and bits_equal(out[0][1], out[1][1])
    assert float(out[0][1].max()) > 0


# ------------------------------------------------------------------------------------------------------ 6. geometry
def test_sphere_mesh_within_the_derived_bound():
    """A constant-depth R = 1 panorama fused into a 24^3 grid over eye +- 1.3 with trunc = 0.3: trunc exceeds the longest
    tetrahedron edge L = sqrt(3) h, so every edge that crosses the sphere has both ends observed and unclamped, where
    tsdf = (R - rho) / trunc.  A vertex is the zero of the linear interpolant of rho - R along such an edge; the second
    derivative of rho along a line is at most 1 / rho <= 1 / (R - L) there, so | |v - eye| - R | <= L^2 / (8 (R - L)) =
    3 h^2 / (8 (R - L)), plus 8 fp32 ulp of the coordinates for the fp32 values and vertices."""
    cam, c2ws, depth, eye, bounds, res = ref.sphere_scene()
    R, trunc = 1.0, 0.3
    vol = volume(res, bounds, trunc)
    vol.integrate(T(depth), cam, c2ws)
    h = max(vol.step)
    L = np.sqrt(3.0) * h
    assert trunc > L
    verts, faces = vol.mesh()
    v, f = N(verts).astype(np.float64), N(faces)
    assert len(v) > 100 and len(f) > 100 and f.min() == 0 and f.max() == len(v) - 1
    eye32 = ref.f32(eye)
    err = np.abs(np.linalg.norm(v - eye32, axis=1) - R)
    bound = 3.0 * h * h / (8.0 * (R - L)) + 8.0 * float(ulp32(np.abs(v).max()))
    print(f"sphere mesh: {len(v)} vertices, {len(f)} faces, worst radial error {err.max():.3e}, bound {bound:.3e}")
    assert err.max() <= bound
    # wound towards free space, which is where the eye is
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    assert (np.einsum("ij,ij->i", np.cross(p1 - p0, p2 - p0), eye32 - p0) > 0).all()
    # every face's cell is fully observed here, so culling changes nothing
    cv, cf = vol.mesh(cull=True)
    assert bits_equal(cv, verts) and bits_equal(cf, faces)
    # unknown = "empty" adds the back shell between the band and the unobserved voxels behind it
    ev, ef = vol.mesh(unknown="empty")
    assert ef.shape[0] > faces.shape[0]
    # ... which culling removes again: its cells have unobserved corners
    kv, kf = vol.mesh(unknown="empty", cull=True)
    assert bits_equal(kv, verts) and bits_equal(kf, faces)


# ------------------------------------------------------------------------------------------------------ 7. plumbing
@functools.lru_cache(maxsize=None)
def model():
    import pano_nerf_amd as pn
    from oracle import pano_oracle as orc
    m = pn.PanoMipNeRF(num_samples=8, rgb_activation="softplus", mlp_num_density_channels=5, num_env_samples=10)
    m.mlp.load_state_dict(orc.init_params(4, 5))
    return m.to(dev())


def test_fuse_views_and_fused_mesh_compose():
    """fuse_views is integrate of render_view's fine_dep, and fused_mesh's normals and colours are query_field's at its
    vertices with the grid's variance: bit for bit."""
    from pano_nerf_amd import fusion, geometry, views
    cam = views.pano_camera(8, 16)
    poses = np.stack([np.eye(4), np.eye(4)])
    poses[1, :3, 3] = (0.1, 0.0, -0.1)
    bounds, res, far = ((-0.6, -0.5, -0.55), (0.5, 0.6, 0.45)), 6, 2.0
    vol = fusion.fuse_views(model(), cam, poses, bounds, res, far=far, depth_max=far, views_per_call=1)
    hand = fusion.TSDFVolume(bounds, res, device="cuda")  # the current device, as a tensor reports it
    assert hand.device == dev()
    assert hand.trunc == float(np.float32(3.0 * max(hand.step)))
    deps = [views.render_view(model(), cam, p, outputs=("depth",), far=far)["fine_dep"] for p in poses]
    for d, p in zip(deps, poses):
        hand.integrate(d, cam, p, depth_max=far)
    assert bits_equal(vol.tsdf, hand.tsdf) and bits_equal(vol.weight, hand.weight)
    assert bool(vol.observed().any())
    # both views in one call is another (equally valid) rounding: one fp32 rounding instead of two
    one = fusion.fuse_views(model(), cam, poses, bounds, res, far=far, depth_max=far)
    assert bits_equal(one.weight, vol.weight)
    assert float((one.tsdf - vol.tsdf).abs().max()) <= 2.0 ** -22
    # the default depth_max = 0.98 far drops what the other one keeps or keeps the same: never sees more
    dflt = fusion.fuse_views(model(), cam, poses, bounds, res, far=far)
    assert bool((dflt.weight <= vol.weight).all())
    mesh = fusion.fused_mesh(model(), vol, colors="albedo")
    verts, faces = vol.mesh()
    assert bits_equal(mesh.vertices, verts) and bits_equal(mesh.faces, faces)
    if verts.shape[0]:
        var = max(vol.step) ** 2 / 12.0
        q = geometry.query_field(model(), verts, var, outputs=("normal", "albedo"))
        assert bits_equal(mesh.normals, q["normal"]) and bits_equal(mesh.colors, q["albedo"])
    again = fusion.fused_mesh(model(), cam, poses, bounds, res, far=far, depth_max=far, views_per_call=1, normals=False,
                              colors=None)
    assert bits_equal(again.vertices, verts) and again.normals is None and again.colors is None


# ------------------------------------------------------------------------------------------------- the C ABI's errors
def test_entry_point_errors():
    from pano_nerf_amd import _lib
    lib = _lib.load()
    OK, SHAPE, UNSUPPORTED, NULL = 0, -1, -2, -3
    z = torch.zeros(8, dtype=torch.float32, device=dev())
    d = torch.ones(2 * 8 * 16, dtype=torch.float32, device=dev())
    m = T(np.stack([np.eye(4)] * 2).reshape(2, 16))
    params = np.zeros(20, np.float32)
    params[:2] = (5.0, 1.5)

    def call(res=(2, 2, 2), S=2, kind=0, H=8, W=16, p=params, c2w=m, depth=d, trunc=0.5, dmax=np.inf, wmax=np.inf, t=z, w=z):
        a = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())
        return lib.pn_tsdf_integrate(*res, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, S, kind, H, W, a(p), a(c2w), a(depth), None, None,
                                     trunc, dmax, wmax, a(t), a(w), _lib.stream(dev()))

    assert call(res=(1, 2, 2)) == SHAPE and call(res=(2048, 1024, 1024)) == SHAPE and call(S=0) == SHAPE
    assert call(H=1) == SHAPE and call(W=2) == SHAPE and call(kind=2, H=12, W=3) == SHAPE and call(kind=1, W=1) == SHAPE
    assert call(S=1 << 20, H=64, W=64) == SHAPE
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert call(trunc=bad) == SHAPE
    for bad in (0.0, -1.0, np.nan):
        assert call(dmax=bad) == SHAPE and call(wmax=bad) == SHAPE
    assert call(kind=3, H=4, W=4, p=np.zeros(20, np.float32)) == SHAPE
    assert call(kind=4) == UNSUPPORTED and call(kind=5) == UNSUPPORTED and call(kind=-1) == UNSUPPORTED
    for name in ("p", "c2w", "depth", "t", "w"):
        assert call(**{name: None}) == NULL
    w = torch.zeros(8, dtype=torch.float32, device=dev())
    assert call(w=w) == OK and call(kind=3, H=16, W=8, w=w) == OK and call(kind=2, H=12, W=2, S=2, w=w) == OK
    torch.cuda.synchronize()
    assert float(w.max()) > 0
