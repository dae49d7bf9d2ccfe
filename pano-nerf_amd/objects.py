"""Virtual object insertion: a synthetic mesh placed into the captured scene, lit by the light that arrives at its
position, hidden by what stands in front of it, and darkening the scene under it.

Everything runs on the HIP device through the kernels of ``libpanonerf_hip.so`` (``pn_objects.hip``, whose one tracer and
one shadow kernel ask ``pn_tri.h``'s finders - brute force, or a walk of ``pn_bvh.hip``'s tree - plus the renderer's and
the lighting module's entry points), under ``torch.no_grad()`` on the current stream.  CPU tensors raise: there is no
host fallback.  No gradients flow through any of it.

    trace_mesh(origins, directions, vertices, faces, t_max, any_hit)   closest hit (t, face, bary) of rays with a mesh
    MeshBVH.build(vertices, faces)                                     a linear BVH over the triangles, built on the device
    shade(probes, albedo, normals, viewdirs, roughness, weights)       the reference's surface_rendering under light probes
    shadow_ratio(points, normals, probe, vertices, faces, bias)        share of a point's irradiance the mesh leaves
    Texture(image, srgb) / Texture.from_file(path, srgb)               a mip-mapped texture on the device (PNG or EXR)
    VirtualObject(vertices, faces, normals, albedo, roughness, ...)    a mesh with its material; from_mesh, from_obj,
                                                                       transformed; uv, face_uv and albedo / roughness /
                                                                       normal maps
    hit_attributes(obj, origins, directions, t, face, bary, ...)       mask, points, normals, albedo, viewdirs, weights
                                                                       (+ roughness with a roughness map)
    sample_textures(obj, mask, face, bary, directions, t, normals)     the texture sampler alone, with the levels it used
    insert_object(model, camera, c2w, obj, ...)                        dict of [1, C, H, W]: the composited frame
    insert_path(model, camera, poses, obj, ...)                        frames of a pose stack (or PNG files)

Conventions (include/panonerf_hip.h states them in full): directions are not normalised and t is in their units, as the
renderer's depth; viewdirs are camera-to-surface and the BRDF sees v = -viewdirs; triangle edges are inclusive with a
band of 2e-6 barycentric units; among equal t the lowest face index wins.  Face indices outside [0, V) are not an error
of trace_mesh / shadow_ratio (checking them would cost a device synchronisation per call): such a face is never hit.
VirtualObject checks them once, when it is built.

trace_mesh and shadow_ratio are brute force over the triangles unless told otherwise: accel=None is that path, untouched.
accel="bvh" builds a MeshBVH for the call and walks it; accel=<a MeshBVH of the same mesh> reuses one (VirtualObject.bvh()
builds it once and keeps it; insert_object / insert_path pass accel on and build once for all frames).  The BVH result
does not depend on the tree and equals brute force wherever no accepted hit lies outside its triangle's padded box (the
header's "candidate rule"): tests/test_bvh_cpu.py shows that no such hit exists on its scenes.  Measured on one MI355X
(profiles/objects_bvh.txt): with the build inside the call the BVH is slower than brute force at 80 faces and below and
faster from 320 on - 63 to 81 times at 81 920 faces, where the two tracers differed on no ray of either test frame.

Texture maps (pn_textures.hip; include/panonerf_hip.h states every formula).  A Texture is one fp32 buffer of float4
texels holding all mip levels (level l is max(1, H >> l) x max(1, W >> l), a 2 x 2 box filter of the level below, clamped
at odd edges); uint8 images are decoded through a 256-entry table (i / 255, or the exact sRGB EOTF with srgb=True).  An
object with uv [T, 2] (and face_uv [F, 3] when the UVs are indexed per corner, as in OBJ files; without it they are per
vertex) takes an albedo_map, a roughness_map (channel 0; needs roughness not None, i.e. the microfacet branch) and a
tangent-space normal_map.  hit_attributes then runs the sampler after the untextured kernel: UV = the barycentric blend;
level of detail = the ray-cone footprint lambda = 0.5 log2(W H A_uv / A_w) + log2(2 radii t) - log2(|n_g . d| / |d|),
clamped to the pyramid (radii=None: level 0), trilinear between the two levels, bilinear within one; wrap="repeat" or
"clamp"; flip_v=True puts V = 0 at the image's last row (the OBJ convention), flip_v=False at its first.  The normal map
perturbs the shading normal N in the frame (T', B', N) that Gram-Schmidt makes of the UV gradients, and keeps N where
that frame does not exist or the result would face away from the eye.  insert_object / insert_path hand the frame rays'
radii on, so a distant or grazing surface reads a coarser level.  An object without maps calls exactly what it called
before.  Out of scope: anisotropic filtering, several materials per object, emissive / metallic maps, texture compression.
"""
import os

import numpy as np
import torch

from . import _lib, views
from .geometry import Mesh, _model_device
from .lighting import _probe_view, _table, light_probes

MAX_PROBES = 8


def _cuda(*named):
    dev = None
    for name, t in named:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor; got {type(t).__name__}")
        if t.device.type != "cuda":
            raise RuntimeError(f"pano_nerf_amd.objects runs on a HIP device only ({name} is on {t.device}); there is no "
                               "CPU fallback")
        if dev is not None and t.device != dev:
            raise RuntimeError(f"tensors are on {dev} and {t.device}")
        dev = t.device
    return dev


def _rows3(t, name, R=None):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be an [R, 3] tensor; got {getattr(t, 'shape', type(t))}")
    if R is not None and t.shape[0] != R:
        raise ValueError(f"{name} has {t.shape[0]} rows; expected {R}")
    return t.detach().to(torch.float32).contiguous()


def _mesh(vertices, faces):
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices must be a [V, 3] tensor; got {getattr(vertices, 'shape', type(vertices))}")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be an [F, 3] tensor; got {getattr(faces, 'shape', type(faces))}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"faces must hold int32 indices; got {faces.dtype}")
    return vertices.detach().to(torch.float32).contiguous(), faces.detach().to(torch.int32).contiguous()


class _PreparedMesh:
    """What a tracer launch reads of one mesh, on the device: tris [F, 12] (pn_tri_setup's rows), bsphere [4] (a sphere
    around the vertices), F and the device; F = 0 has no tensors.  As it is, it traces by brute force (nodes stays None):
    accel=None makes one per call.  With a tree it is a MeshBVH."""

    def __init__(self, tris, nodes, bsphere, F, device):
        self.tris, self.nodes, self.bsphere, self.F, self.device = tris, nodes, bsphere, F, device

    def _entry(self, name):
        """(the entry point that traces this mesh, the arguments it takes after tris)"""
        return name, ()


class MeshBVH(_PreparedMesh):
    """A linear BVH over the triangles of one mesh, on the device: tris [F, 12] (the tracer's rows), nodes
    [max(F - 1, 1), 16] (both children's boxes and references per row; include/panonerf_hip.h), bsphere [4], F and the
    device.  Build it with MeshBVH.build; hand it to trace_mesh / shadow_ratio / insert_object as `accel`."""

    @classmethod
    def build(cls, vertices, faces):
        """Padded triangle boxes -> 63-bit Morton keys -> torch.sort (stable) -> Karras' radix tree -> bottom-up refit, all
        launched on the current stream without a host synchronisation.  Two builds of a mesh give the same bytes."""
        dev = _cuda(("vertices", vertices), ("faces", faces))
        with torch.no_grad(), torch.cuda.device(dev):
            return _prepare(*_mesh(vertices, faces), dev, "bvh")

    def _entry(self, name):
        return (name + "_bvh", (self.nodes.data_ptr(),)) if self.F else (name, ())  # nothing to hit: no tree either


def _check_accel(accel):
    """accel is None, "bvh" or a MeshBVH: anything else raises before a tensor is looked at."""
    if accel is None or isinstance(accel, MeshBVH) or (isinstance(accel, str) and accel == "bvh"):
        return
    raise ValueError(f'accel must be None (brute force), "bvh" or a MeshBVH; got {accel!r}')


def _prepare(v, f, dev, accel):
    """The mesh a call launches on, of the tensors _mesh returns: the tracer's rows and a sphere around the vertices, made
    for this call (accel=None: brute force), with a tree built for it ("bvh"), or the MeshBVH handed in.  Of a tree handed
    in only the face count and the device are compared with the mesh: keeping the two in step is the caller's business
    (VirtualObject.bvh() does).  Launches on the current stream."""
    F = int(f.shape[0]) if v.shape[0] else 0  # no vertices: nothing to hit
    cls = _PreparedMesh if accel is None else MeshBVH
    if not F:
        return cls(None, None, None, 0, dev)
    if isinstance(accel, MeshBVH):
        if accel.F != F or accel.device != dev:
            raise ValueError(f"accel is a MeshBVH of {accel.F} faces on {accel.device}; the mesh has {F} on {dev}")
        return accel
    st = _lib.stream(dev)
    tris = torch.empty(F, 12, dtype=torch.float32, device=dev)
    _lib.call("pn_tri_setup", F, int(v.shape[0]), v.data_ptr(), f.data_ptr(), tris.data_ptr(), st)
    lo, hi = v.amin(0), v.amax(0)
    centre = (lo + hi) * 0.5
    radius = (v - centre).norm(dim=1).amax().reshape(1)
    bsphere = torch.cat([centre, radius]).contiguous()
    if accel is None:
        return cls(tris, None, bsphere, F, dev)
    tbox = torch.empty(F, 2, 4, dtype=torch.float32, device=dev)
    _lib.call("pn_bvh_boxes", F, int(v.shape[0]), v.data_ptr(), f.data_ptr(), tbox.data_ptr(), st)
    nodes = torch.empty(max(F - 1, 1), 16, dtype=torch.float32, device=dev)
    if F == 1:
        _lib.call("pn_bvh_tree", F, None, None, tbox.data_ptr(), nodes.data_ptr(), None, None, st)
        return cls(tris, nodes, bsphere, F, dev)
    scene = torch.cat([tbox[:, 0, :3].amin(0), tbox[:, 1, :3].amax(0)]).contiguous()
    keys = torch.empty(F, dtype=torch.int64, device=dev)
    _lib.call("pn_bvh_keys", F, tbox.data_ptr(), scene.data_ptr(), keys.data_ptr(), st)
    skeys, order = torch.sort(keys, stable=True)
    leaf_parent = torch.empty(F, dtype=torch.int32, device=dev)
    counters = torch.empty(F - 1, dtype=torch.int32, device=dev)
    _lib.call("pn_bvh_tree", F, skeys.data_ptr(), order.data_ptr(), tbox.data_ptr(), nodes.data_ptr(),
              leaf_parent.data_ptr(), counters.data_ptr(), st)
    return cls(tris, nodes, bsphere, F, dev)


def trace_mesh(origins, directions, vertices, faces, t_max=None, any_hit=False, accel=None):
    """Closest intersection of the R rays o + t d (fp32 [R, 3]; d is not normalised, t is in its units) with the F
    triangles of (vertices [V, 3], faces [F, 3] int32), two-sided: (t [R], +inf for a miss; face [R] int32, -1; bary
    [R, 2] = Moeller-Trumbore's (u, v), hit = (1 - u - v) v0 + u v1 + v v2).  A hit has t > 0 and t < t_max[r] where
    t_max [R] is given.  any_hit=True returns only a bool [R].  accel=None: brute force over the triangles, streamed through
    LDS.  accel="bvh" or a MeshBVH of this mesh: a BVH walk (the module docstring says what it promises)."""
    _check_accel(accel)
    dev = _cuda(("origins", origins), ("directions", directions), ("vertices", vertices), ("faces", faces),
                ("t_max", t_max))
    o = _rows3(origins, "origins")
    R = int(o.shape[0])
    d = _rows3(directions, "directions", R)
    v, f = _mesh(vertices, faces)
    tm = None
    if t_max is not None:
        if t_max.numel() != R:
            raise ValueError(f"t_max must hold {R} values; got {tuple(t_max.shape)}")
        tm = t_max.detach().to(torch.float32).reshape(R).contiguous()
    with torch.no_grad(), torch.cuda.device(dev):
        if any_hit:
            hit = torch.zeros(R, dtype=torch.uint8, device=dev)
            t = face = bary = None
        else:
            hit = None
            t = torch.full((R,), float("inf"), dtype=torch.float32, device=dev)
            face = torch.full((R,), -1, dtype=torch.int32, device=dev)
            bary = torch.zeros(R, 2, dtype=torch.float32, device=dev)
        mesh = _prepare(v, f, dev, accel) if R else None
        if R and mesh.F:
            name, nodes = mesh._entry("pn_trace_mesh")
            sphere = () if nodes else (mesh.bsphere.data_ptr(),)  # a walk has its boxes: pn_trace_mesh_bvh takes no sphere
            _lib.call(name, R, o.data_ptr(), d.data_ptr(), mesh.F, mesh.tris.data_ptr(), *nodes, _lib.ptr(tm), *sphere,
                      int(bool(any_hit)), _lib.ptr(t), _lib.ptr(face), _lib.ptr(bary), _lib.ptr(hit), _lib.stream(dev))
    return hit.bool() if any_hit else (t, face, bary)


def shade(probes, albedo, normals, viewdirs, roughness=None, weights=None):
    """The reference's surface_rendering (utils/surface_rendering.py) with the pixels of light probes as the lights:
    (rgb, diffuse, specular, shading), each [R, 3] (shading is None in the microfacet branch, as upstream).

    probes [K, 3, H, W] (1 <= K <= 8; the strided views light_probes returns are read in place); albedo, normals (unit),
    viewdirs [R, 3]: viewdirs point from the camera to the surface and the BRDF is evaluated with v = -viewdirs.
    roughness None: the Lambertian branch.  A float or an [R, 1] tensor: the microfacet branch (microfeast_brdf).
    weights [R, K] blend the probes per row (required for K > 1): the light is sum_k weights[r, k] L_k."""
    x, sp, sc, sw, K, H, W = _probe_view(probes)
    if K > MAX_PROBES:
        raise ValueError(f"shade blends at most {MAX_PROBES} probes; got {K}")
    rough_t = roughness if isinstance(roughness, torch.Tensor) else None
    dev = _cuda(("probes", x), ("albedo", albedo), ("normals", normals), ("viewdirs", viewdirs), ("roughness", rough_t),
                ("weights", weights))
    a = _rows3(albedo, "albedo")
    R = int(a.shape[0])
    n, vd = _rows3(normals, "normals", R), _rows3(viewdirs, "viewdirs", R)
    rough_all = 0.0
    if rough_t is not None:
        if rough_t.numel() != R or rough_t.dim() > 2:
            raise ValueError(f"roughness must be a float or an [R, 1] tensor; got {tuple(rough_t.shape)}")
        rough_t = rough_t.detach().to(torch.float32).reshape(R).contiguous()
    elif roughness is not None:
        rough_all = float(roughness)
    if weights is None:
        if K != 1:
            raise ValueError(f"{K} probes need weights [R, {K}]")
        w = None
    else:
        if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (R, K):
            raise ValueError(f"weights must be [{R}, {K}]; got {getattr(weights, 'shape', type(weights))}")
        w = weights.detach().to(torch.float32).contiguous()
    micro = roughness is not None
    with torch.no_grad(), torch.cuda.device(dev):
        dirs, omega = _table(H, W, dev)
        rgb, diffuse, specular = (torch.empty(R, 3, dtype=torch.float32, device=dev) for _ in range(3))
        shading = None if micro else torch.empty(R, 3, dtype=torch.float32, device=dev)
        if R:
            _lib.call("pn_shade", R, K, H, W, x.data_ptr(), sp, sc, sw, dirs.data_ptr(), omega.data_ptr(), a.data_ptr(),
                      n.data_ptr(), vd.data_ptr(), _lib.ptr(rough_t), rough_all, int(micro), _lib.ptr(w), rgb.data_ptr(),
                      diffuse.data_ptr(), specular.data_ptr(), _lib.ptr(shading), _lib.stream(dev))
    return rgb, diffuse, specular, shading


def shadow_ratio(points, normals, probe, vertices, faces, bias=1e-3, accel=None):
    """[R] fp32 in [0, 1]: the share of the irradiance of scene points [R, 3] (unit normals [R, 3]) that the mesh leaves,
    under one probe [3, H, W] (or [1, 3, H, W]): E(unoccluded pixels) / E(all pixels), E(S) = sum over the probe pixels in
    S of mean_c L(pix) max(0, n . l_pix) omega_pix; a pixel is occluded when the ray from x + bias n along l_pix hits the
    mesh.  1 where E(all) is 0 or the point is not finite.  One fused kernel; meant for a coarse probe (8 x 16).
    accel as in trace_mesh: with a BVH only the occlusion query changes, the sums and their order do not."""
    _check_accel(accel)
    if isinstance(probe, torch.Tensor) and probe.dim() == 3:
        probe = probe[None]
    x, _, sc, sw, P, H, W = _probe_view(probe)
    if P != 1:
        raise ValueError(f"shadow_ratio takes one probe; got {P}")
    dev = _cuda(("probe", x), ("points", points), ("normals", normals), ("vertices", vertices), ("faces", faces))
    p = _rows3(points, "points")
    R = int(p.shape[0])
    n = _rows3(normals, "normals", R)
    v, f = _mesh(vertices, faces)
    with torch.no_grad(), torch.cuda.device(dev):
        dirs, omega = _table(H, W, dev)
        out = torch.empty(R, dtype=torch.float32, device=dev)
        if R:
            mesh = _prepare(v, f, dev, accel)
            name, nodes = mesh._entry("pn_shadow_ratio")
            _lib.call(name, R, H, W, x.data_ptr(), sc, sw, dirs.data_ptr(), omega.data_ptr(), p.data_ptr(), n.data_ptr(),
                      float(bias), mesh.F, _lib.ptr(mesh.tris), *nodes, _lib.ptr(mesh.bsphere), out.data_ptr(), _lib.stream(dev))
    return out


def _decode_table(srgb):
    """256 fp32 values: i / 255 or the sRGB EOTF of it, built in fp64 and rounded once."""
    c = np.arange(256, dtype=np.float64) / 255.0
    if srgb:
        c = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    return c.astype(np.float32)


class Texture:
    """A mip-mapped texture on the device: `data` [sum_l h_l w_l, 4] fp32 (every level, level 0 first; unused channels 0,
    alpha 1), H, W, L = 1 + floor(log2(max(H, W))) and C, the channels of the image it was made from.

    image: uint8 or floating [H, W] / [H, W, C] (C = 1, 3 or 4; 1 <= H, W <= 16384), a host array or a device tensor.
    srgb=True decodes uint8 colour channels with the sRGB EOTF (albedo images); False is i / 255 (roughness and normal
    maps).  A floating image is linear: srgb=True raises.  Built by pn_tex_ingest and pn_tex_pyramid on the current
    stream."""

    def __init__(self, image, srgb=False, device=None):
        if isinstance(image, torch.Tensor):
            dev = image.device
            img = image.detach()
        else:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
            a = np.asarray(image)
            if a.dtype != np.uint8:
                if a.dtype.kind != "f":
                    raise ValueError(f"a texture image must be uint8 or floating; got {a.dtype}")
                a = a.astype(np.float32)
            img = torch.from_numpy(np.ascontiguousarray(a))
        if dev.type != "cuda":
            raise RuntimeError(f"pano_nerf_amd.objects runs on a HIP device only (the texture is on {dev}); there is no CPU "
                               "fallback")
        if img.dim() == 2:
            img = img[:, :, None]
        if img.dim() != 3 or img.shape[2] not in (1, 3, 4) or not (1 <= img.shape[0] <= 16384 and 1 <= img.shape[1] <= 16384):
            raise ValueError(f"a texture image must be [H, W] or [H, W, C] with C in (1, 3, 4) and 1 <= H, W <= 16384; got "
                             f"{tuple(img.shape)}")
        is_u8 = img.dtype == torch.uint8
        if not is_u8 and not img.dtype.is_floating_point:
            raise ValueError(f"a texture image must be uint8 or floating; got {img.dtype}")
        if srgb and not is_u8:
            raise ValueError("srgb=True decodes uint8 images; a floating image is taken as linear")
        img = (img if is_u8 else img.to(torch.float32)).to(dev).contiguous()
        self.H, self.W, self.C = (int(x) for x in img.shape)
        self.L = 1 + int(max(self.H, self.W)).bit_length() - 1
        self.srgb, self.device = bool(srgb), dev
        with torch.no_grad(), torch.cuda.device(dev):
            n = _lib.load().pn_tex_floats(self.H, self.W)
            if n < 0:
                _lib.check(int(n), "pn_tex_floats")
            self.data = torch.empty(n // 4, 4, dtype=torch.float32, device=dev)
            table = torch.from_numpy(_decode_table(srgb)).to(dev) if is_u8 else None
            _lib.call("pn_tex_ingest", self.H, self.W, self.C, int(is_u8), img.data_ptr(), _lib.ptr(table),
                      self.data.data_ptr(), _lib.stream(dev))
            _lib.call("pn_tex_pyramid", self.H, self.W, self.data.data_ptr(), _lib.stream(dev))
            for x in (img, table):  # the launches above read them on this stream
                if x is not None:
                    x.record_stream(torch.cuda.current_stream(dev))

    @classmethod
    def from_file(cls, path, srgb=False, device=None):
        """A .png (io_exr.read_png; a grey + alpha file keeps its grey channel) or .exr (io_exr.read_exr: RGB, always
        linear, whatever srgb says) file."""
        from . import io_exr
        ext = os.path.splitext(path)[1].lower()
        if ext == ".png":
            img = io_exr.read_png(path)
            if img.ndim == 3 and img.shape[2] == 2:
                img = img[:, :, 0]
            return cls(img, srgb=srgb, device=device)
        if ext == ".exr":
            return cls(io_exr.read_exr(path), srgb=False, device=device)
        raise ValueError(f"{path}: textures are read from .png and .exr files; got {ext!r}")

    def level_shape(self, l):
        """(texel offset, h_l, w_l) of level l"""
        if not 0 <= l < self.L:
            raise ValueError(f"level {l} outside the {self.L} levels of a {self.H} x {self.W} texture")
        off = sum(max(1, self.H >> i) * max(1, self.W >> i) for i in range(l))
        return off, max(1, self.H >> l), max(1, self.W >> l)

    def level(self, l):
        """A view [h_l, w_l, 4] of level l."""
        off, h, w = self.level_shape(l)
        return self.data[off:off + h * w].view(h, w, 4)


_WRAP = {"repeat": 0, "clamp": 1}


class VirtualObject:
    """A triangle mesh with its material, on the device.  vertices [V, 3], faces [F, 3] int32 (device tensors or arrays
    on the host, which are copied to `device`); normals: per vertex (interpolated with the barycentrics and renormalised)
    or None (the geometric normalize(e1 x e2)); albedo: one colour or [V, 3] (e.g. Mesh.colors); roughness: None
    (Lambertian) or a float (microfacet).  The shading normal is flipped towards the eye.  Face indices are checked here.
    Texture maps (the module docstring has the conventions): uv [T, 2]; face_uv [F, 3] int32 indexes it per corner (None:
    T = V and faces index it); albedo_map replaces the albedo, roughness_map (channel 0; needs roughness not None, which
    selects the microfacet branch) the roughness per hit, normal_map perturbs the shading normal; wrap "repeat" or "clamp";
    flip_v=True (OBJ's convention) puts V = 0 at the image's last row.  A map without uv raises; face_uv is checked here."""

    def __init__(self, vertices, faces, normals=None, albedo=(0.8, 0.8, 0.8), roughness=None, device=None, uv=None,
                 face_uv=None, albedo_map=None, roughness_map=None, normal_map=None, wrap="repeat", flip_v=True):
        dev = None
        for t in (vertices, faces, normals, albedo, uv, face_uv):
            if isinstance(t, torch.Tensor):
                dev = t.device
                break
        if dev is None:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError(f"pano_nerf_amd.objects runs on a HIP device only (the object is on {dev}); there is no CPU "
                               "fallback")
        to = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).to(device=dev, dtype=dt)
        self.vertices, self.faces = _mesh(to(vertices, torch.float32), to(faces, torch.int32))
        V = int(self.vertices.shape[0])
        if self.faces.numel() and (int(self.faces.min()) < 0 or int(self.faces.max()) >= V):
            raise ValueError(f"faces index outside the {V} vertices")
        self.normals = None
        if normals is not None:
            self.normals = to(normals, torch.float32).contiguous()
            if tuple(self.normals.shape) != (V, 3):
                raise ValueError(f"normals must be [V, 3] like the vertices; got {tuple(self.normals.shape)}")
        self.albedo, self.vertex_albedo = None, None
        if isinstance(albedo, torch.Tensor) or np.ndim(albedo) == 2:
            self.vertex_albedo = to(albedo, torch.float32).contiguous()
            if tuple(self.vertex_albedo.shape) != (V, 3):
                raise ValueError(f"albedo must be one colour or [V, 3]; got {tuple(self.vertex_albedo.shape)}")
        else:
            a = np.asarray(albedo, dtype=np.float64).reshape(-1)
            if a.shape != (3,):
                raise ValueError(f"albedo must be one colour or [V, 3]; got shape {np.shape(albedo)}")
            self.albedo = tuple(float(c) for c in a)
        self.roughness = None if roughness is None else float(roughness)
        self.device = dev
        self._bvh, self._bvh_stamp = None, None
        self.uv, self.face_uv = None, None
        if uv is not None:
            self.uv = to(uv, torch.float32).contiguous()
            if self.uv.dim() != 2 or self.uv.shape[1] != 2:
                raise ValueError(f"uv must be [T, 2]; got {tuple(self.uv.shape)}")
            T = int(self.uv.shape[0])
            if face_uv is None:
                if T != V:
                    raise ValueError(f"uv without face_uv is per vertex: it must be [{V}, 2]; got {tuple(self.uv.shape)}")
            else:
                fu = to(face_uv, torch.int64)
                if tuple(fu.shape) != tuple(self.faces.shape):
                    raise ValueError(f"face_uv must be [F, 3] like the faces; got {tuple(fu.shape)}")
                if fu.numel() and (int(fu.min()) < 0 or int(fu.max()) >= T):
                    raise ValueError(f"face_uv index outside the {T} uv rows")
                self.face_uv = fu.to(torch.int32).contiguous()
        elif face_uv is not None:
            raise ValueError("face_uv needs uv")
        if wrap not in _WRAP:
            raise ValueError(f'wrap must be "repeat" or "clamp"; got {wrap!r}')
        self.wrap, self.flip_v = wrap, bool(flip_v)
        self.albedo_map, self.roughness_map, self.normal_map = albedo_map, roughness_map, normal_map
        for name, tex, need in (("albedo_map", albedo_map, 3), ("roughness_map", roughness_map, 1),
                                ("normal_map", normal_map, 3)):
            if tex is None:
                continue
            if not isinstance(tex, Texture):
                raise ValueError(f"{name} must be a Texture; got {type(tex).__name__}")
            if self.uv is None:
                raise ValueError(f"{name} needs uv")
            if tex.device != dev:
                raise RuntimeError(f"{name} is on {tex.device}, the object on {dev}")
            if tex.C < need:
                raise ValueError(f"{name} needs {need} channels; the texture has {tex.C}")
        if roughness_map is not None and self.roughness is None:
            raise ValueError("roughness_map needs roughness not None: a float selects the microfacet branch, in which the "
                             "map gives the per-hit values")

    @property
    def textured(self):
        return self.albedo_map is not None or self.roughness_map is not None or self.normal_map is not None

    def _texture_kw(self):
        return dict(uv=self.uv, face_uv=self.face_uv, albedo_map=self.albedo_map, roughness_map=self.roughness_map,
                    normal_map=self.normal_map, wrap=self.wrap, flip_v=self.flip_v)

    @classmethod
    def from_obj(cls, path, material=None, device=None):
        """The object of a Wavefront OBJ file (geometry.read_obj): the faces of one material, with its Kd as the albedo
        (0.8 grey without one), its Pr as the roughness (with a map_Pr but no Pr: 1.0, so the map gives the values as
        they are), and its maps - map_Kd (decoded as sRGB when it is a PNG), map_Pr, and norm / map_Bump / bump as the
        normal map - loaded relative to the MTL file.  material=None takes the only material (or all faces when the file
        names none); with several it raises, naming them.  UVs keep OBJ's convention (flip_v=True, wrap="repeat")."""
        from .geometry import read_obj
        m = read_obj(path)
        names = list(m.materials)
        used = sorted(set(int(i) for i in m.face_material))
        if material is None:
            if len(used) > 1:
                raise ValueError(f"{path} uses {len(used)} materials "
                                 f"({', '.join(repr(names[i]) if i >= 0 else '<none>' for i in used)}): pass material=")
            pick = used[0] if used else -1
        else:
            if material not in names:
                raise ValueError(f"{path} has no material {material!r}; it has {names}")
            pick = names.index(material)
        keep = m.face_material == pick
        if not keep.any():
            raise ValueError(f"{path}: no face uses material {material!r}")
        mat = m.materials[names[pick]] if pick >= 0 else dict(Kd=None, Pr=None, map_Kd=None, map_Pr=None, norm=None)
        rough = mat["Pr"] if mat["Pr"] is not None else (1.0 if mat["map_Pr"] else None)
        tex = lambda p, srgb: None if p is None else Texture.from_file(p, srgb=srgb, device=device)
        has_uv = m.uv is not None
        for key in ("map_Kd", "map_Pr", "norm"):
            if mat[key] and not has_uv:
                raise ValueError(f"{path}: material {names[pick]!r} has {key} but the faces carry no vt")
        return cls(m.vertices, m.faces[keep], m.normals, mat["Kd"] or (0.8, 0.8, 0.8), rough, device,
                   uv=m.uv, face_uv=m.face_uv[keep] if has_uv else None, albedo_map=tex(mat["map_Kd"], True),
                   roughness_map=tex(mat["map_Pr"], False), normal_map=tex(mat["norm"], False))

    @classmethod
    def from_mesh(cls, mesh, albedo=None, roughness=None, device=None):
        """The object of a geometry.Mesh: its normals, and its colours as the albedo unless one is given."""
        if albedo is None:
            albedo = mesh.colors if mesh.colors is not None else (0.8, 0.8, 0.8)
        return cls(mesh.vertices, mesh.faces, mesh.normals, albedo, roughness, device)

    @classmethod
    def from_baked(cls, baked, roughness=None):
        """The object of a geometry.BakedMesh: its atlas UVs, its "albedo" map ("radiance" without one) as the albedo
        texture and its "normal" map as the normal map, built from the fp32 images as they are (no 8-bit step).  Sample
        it at level 0 (hit_attributes(radii=None)): the higher mip levels of a per-triangle atlas mix faces."""
        col = baked.maps.get("albedo", baked.maps.get("radiance"))
        nrm = baked.maps.get("normal")
        return cls(baked.vertices, baked.faces, baked.normals, (0.8, 0.8, 0.8), roughness, uv=baked.uv,
                   face_uv=baked.face_uv, albedo_map=None if col is None else Texture(col),
                   normal_map=None if nrm is None else Texture(nrm))

    def transformed(self, matrix):
        """The object moved by a 4x4 matrix (points: M x; normals: the inverse transpose of its 3x3 part, renormalised).
        UVs and texture maps come along (the Texture objects are shared, not copied)."""
        m = np.asarray(matrix, dtype=np.float64)
        if m.shape != (4, 4) or not np.isfinite(m).all():
            raise ValueError(f"matrix must be a finite 4x4 matrix; got shape {m.shape}")
        a = torch.from_numpy(m[:3, :3].T.astype(np.float32)).to(self.device)
        v = self.vertices @ a + torch.from_numpy(m[:3, 3].astype(np.float32)).to(self.device)
        n = None
        if self.normals is not None:
            it = torch.from_numpy(np.linalg.inv(m[:3, :3]).astype(np.float32)).to(self.device)  # (M^-T n)^T = n^T M^-1
            n = torch.nn.functional.normalize(self.normals @ it, dim=1)
        return VirtualObject(v, self.faces, n, self.vertex_albedo if self.vertex_albedo is not None else self.albedo,
                             self.roughness, **self._texture_kw())

    def bvh(self):
        """The MeshBVH of this object, built on first use and kept for as long as vertices and faces are the tensors it
        was built from, unchanged (their storage and torch's in-place version counters are compared, on the host): an
        assignment or an in-place edit of either builds anew.  transformed() returns an object without one."""
        stamp = tuple(x for t in (self.vertices, self.faces) for x in (t.data_ptr(), tuple(t.shape), t._version))
        if self._bvh is None or self._bvh_stamp != stamp:
            self._bvh, self._bvh_stamp = MeshBVH.build(self.vertices, self.faces), stamp
        return self._bvh

    def centroid(self):
        """[1, 3]: the mean of the vertices."""
        return self.vertices.mean(0, keepdim=True)


def _positions(obj, probe_positions, dev):
    if probe_positions is None:
        return obj.centroid()
    if not isinstance(probe_positions, torch.Tensor):
        probe_positions = torch.as_tensor(np.asarray(probe_positions, dtype=np.float32)).to(dev)
    if probe_positions.dim() != 2 or probe_positions.shape[1] != 3 or not 1 <= probe_positions.shape[0] <= MAX_PROBES:
        raise ValueError(f"probe_positions must be [K, 3] with 1 <= K <= {MAX_PROBES}; got {tuple(probe_positions.shape)}")
    _cuda(("probe_positions", probe_positions))
    return probe_positions.detach().to(torch.float32).contiguous()


def _texture_hits(obj, R, mask, face, bary, d, t, normals_in, radii, albedo, roughness, normals, lod, dev):
    """pn_texture_hits on prepared (fp32 / int32 / uint8, contiguous) tensors; outputs of absent maps are not touched"""
    if not R:
        return
    tex = []
    for m in (obj.albedo_map, obj.roughness_map, obj.normal_map):
        tex += [None, 0, 0] if m is None else [m.data.data_ptr(), m.H, m.W]
    _lib.call("pn_texture_hits", R, mask.data_ptr(), face.data_ptr(), bary.data_ptr(), d.data_ptr(), t.data_ptr(),
              normals_in.data_ptr(), _lib.ptr(radii), int(obj.vertices.shape[0]), obj.vertices.data_ptr(),
              int(obj.faces.shape[0]), obj.faces.data_ptr(), int(obj.uv.shape[0]), obj.uv.data_ptr(),
              _lib.ptr(obj.face_uv), *tex, _WRAP[obj.wrap], int(obj.flip_v), _lib.ptr(albedo), _lib.ptr(roughness),
              _lib.ptr(normals), _lib.ptr(lod), _lib.stream(dev))


def _hit_rows(R, t, face, bary, radii, scene_dep, mismatch):
    """(t [R], face [R] int32, bary [R, 2], radii [R] or None, scene_dep [R] or None) as the kernels read them: fp32 /
    int32, contiguous.  mismatch: the caller's message for a t, face or bary of another length."""
    if t.numel() != R or face.numel() != R or tuple(bary.shape) != (R, 2):
        raise ValueError(mismatch)
    tt = t.detach().to(torch.float32).reshape(R).contiguous()
    ff = face.detach().to(torch.int32).reshape(R).contiguous()
    bb = bary.detach().to(torch.float32).contiguous()
    dep = rad = None
    if scene_dep is not None:
        if scene_dep.numel() != R:
            raise ValueError(f"scene_dep must hold {R} values; got {tuple(scene_dep.shape)}")
        dep = scene_dep.detach().to(torch.float32).reshape(R).contiguous()
    if radii is not None:
        if radii.numel() != R or radii.dim() > 2:
            raise ValueError(f"radii must be [R] or [R, 1] with R = {R}; got {tuple(radii.shape)}")
        rad = radii.detach().to(torch.float32).reshape(R).contiguous()
    return tt, ff, bb, rad, dep


def sample_textures(obj, mask, face, bary, directions, t, normals, radii=None):
    """The texture sampler on its own, at hits given by hand: mask [R] bool, face [R] int32, bary [R, 2], directions
    [R, 3], t [R], normals [R, 3] (the shading normals, facing the eye), radii [R] / [R, 1] or None.  Returns a dict with
    albedo [R, 3], roughness [R, 1] and normals [R, 3] - each only when the object has that map - and lod [R, 3], the level
    of detail used per map (albedo, roughness, normal; 0 for an absent one).  Rows outside the mask are 0.
    hit_attributes runs exactly this after the untextured attributes."""
    if not isinstance(obj, VirtualObject) or not obj.textured:
        raise ValueError("sample_textures needs a VirtualObject with at least one texture map")
    dev = _cuda(("mask", mask), ("face", face), ("bary", bary), ("directions", directions), ("t", t), ("normals", normals),
                ("radii", radii), ("vertices", obj.vertices))
    d = _rows3(directions, "directions")
    R = int(d.shape[0])
    n = _rows3(normals, "normals", R)
    mismatch = f"mask, t, face [R] and bary [R, 2] must match the {R} rows"
    if mask.numel() != R:
        raise ValueError(mismatch)
    tt, ff, bb, rad, _ = _hit_rows(R, t, face, bary, radii, None, mismatch)
    m8 = mask.detach().reshape(R).to(torch.uint8).contiguous()
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        out = dict(lod=e(R, 3))
        if obj.albedo_map is not None:
            out["albedo"] = e(R, 3)
        if obj.roughness_map is not None:
            out["roughness"] = e(R, 1)
        if obj.normal_map is not None:
            out["normals"] = e(R, 3)
        _texture_hits(obj, R, m8, ff, bb, d, tt, n, rad, out.get("albedo"), out.get("roughness"), out.get("normals"),
                      out["lod"], dev)
    return out


def hit_attributes(obj, origins, directions, t, face, bary, scene_dep=None, probe_positions=None, radii=None):
    """What shade needs at the hits trace_mesh found, as a dict of per-ray tensors: mask [R] bool (hit, and not
    t >= scene_dep where scene_dep [R] is given: a NaN depth counts as behind), points = o + t d, normals (interpolated
    or geometric, flipped towards the eye), albedo, viewdirs = d / |d| [R, 3] and weights [R, K] (normalised inverse
    distances of the point to probe_positions [K, 3]; a point within 1e-6 of a position takes that probe alone); rows
    outside the mask are 0.  With scene_dep also scene_points [R, 3] = o + scene_dep d outside the mask and NaN inside:
    the points insert_object hands to shadow_ratio (a NaN point's ratio is 1).
    An object with texture maps: the same call, then the sampler (pn_texture_hits) on its outputs - an albedo_map replaces
    the albedo rows, a normal_map the normals rows, a roughness_map adds roughness [R, 1].  radii ([R] or [R, 1], the
    renderer's per-ray cone radii: the footprint at the hit is 2 radii t wide) picks the mip level; None samples level 0.
    An object without maps ignores radii."""
    if not isinstance(obj, VirtualObject):
        raise ValueError(f"obj must be a VirtualObject; got {type(obj).__name__}")
    dev = _cuda(("origins", origins), ("directions", directions), ("t", t), ("face", face), ("bary", bary),
                ("scene_dep", scene_dep), ("vertices", obj.vertices), ("radii", radii))
    o = _rows3(origins, "origins")
    R = int(o.shape[0])
    d = _rows3(directions, "directions", R)
    tt, ff, bb, rad, dep = _hit_rows(R, t, face, bary, radii, scene_dep,
                                     f"t, face [R] and bary [R, 2] must match the {R} rays")
    pos = None if probe_positions is None else _positions(obj, probe_positions, dev)
    K = 1 if pos is None else int(pos.shape[0])
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        mask = torch.zeros(R, dtype=torch.uint8, device=dev)
        out = dict(points=e(R, 3), normals=e(R, 3), albedo=e(R, 3), viewdirs=e(R, 3))
        weights = e(R, K) if pos is not None else None
        spoints = e(R, 3) if dep is not None else None
        col = obj.albedo or (0.0, 0.0, 0.0)
        if R:
            _lib.call("pn_object_hits", R, o.data_ptr(), d.data_ptr(), tt.data_ptr(), ff.data_ptr(), bb.data_ptr(),
                      _lib.ptr(dep), int(obj.vertices.shape[0]), obj.vertices.data_ptr(), int(obj.faces.shape[0]),
                      obj.faces.data_ptr(), _lib.ptr(obj.normals), _lib.ptr(obj.vertex_albedo), *col, K, _lib.ptr(pos),
                      mask.data_ptr(), out["points"].data_ptr(), out["normals"].data_ptr(), out["albedo"].data_ptr(),
                      out["viewdirs"].data_ptr(), _lib.ptr(weights), _lib.ptr(spoints), _lib.stream(dev))
        if obj.textured:
            rough = e(R) if obj.roughness_map is not None else None
            _texture_hits(obj, R, mask, ff, bb, d, tt, out["normals"], rad, out["albedo"], rough, out["normals"], None, dev)
            if rough is not None:
                out["roughness"] = rough.reshape(R, 1)
    out["mask"] = mask.bool()
    if weights is not None:
        out["weights"] = weights
    if spoints is not None:
        out["scene_points"] = spoints
    return out


def _frame_rays(camera, c2w, near, far, dev):
    """(origins, directions [H W, 3], cone radii [H W, 1]) of the rays render_view renders for this camera and pose."""
    rays = views.generate_camera_rays(camera, c2w, near, far, dev)
    return rays.origins, rays.directions, rays.radii


def _insert(model, camera, c2w, obj, pos, probes, shadow_probe, shadow_bias, near, far, chunk_rays, accel=None):
    dev = _model_device(model)
    H, W = camera.h, camera.w
    R = H * W
    scene = views.render_view(model, camera, c2w, outputs=("rgb", "depth", "normal"), near=near, far=far,
                              chunk_rays=chunk_rays)
    rows = lambda x: x.permute(0, 2, 3, 1).reshape(R, -1)  # the [H W, C] buffer behind a render_view output
    s_rgb, s_dep, s_nor = rows(scene["fine_rgb"]), rows(scene["fine_dep"]), rows(scene["fine_nor"])
    with torch.no_grad(), torch.cuda.device(dev):
        o, d, radii = _frame_rays(camera, c2w, near, far, dev)
        t, face, bary = trace_mesh(o, d, obj.vertices, obj.faces, accel=accel)
        K = int(pos.shape[0])
        at = hit_attributes(obj, o, d, t, face, bary, s_dep, pos if K > 1 else None, radii=radii)
        mask = at["mask"]
        object_rgb = torch.zeros(R, 3, dtype=torch.float32, device=dev)
        hit = torch.nonzero(mask).reshape(-1)  # the one host synchronisation: sizes the shading launch
        if hit.numel():
            g = lambda x: x.index_select(0, hit)
            rough = g(at["roughness"]) if "roughness" in at else obj.roughness
            rgb_hit = shade(probes, g(at["albedo"]), g(at["normals"]), g(at["viewdirs"]), rough,
                            g(at["weights"]) if K > 1 else None)[0]
            object_rgb.index_copy_(0, hit, rgb_hit)
        if shadow_probe is not None:
            shadow = shadow_ratio(at["scene_points"], s_nor, shadow_probe, obj.vertices, obj.faces, shadow_bias,
                                  accel=accel)
        else:
            shadow = torch.ones(R, dtype=torch.float32, device=dev)
        rgb = torch.empty(R, 3, dtype=torch.float32, device=dev)
        depth = torch.empty(R, dtype=torch.float32, device=dev)
        m8 = mask.to(torch.uint8)
        _lib.call("pn_object_composite", R, m8.data_ptr(), object_rgb.data_ptr(), t.data_ptr(), s_rgb.data_ptr(),
                  s_dep.reshape(R).data_ptr(), shadow.data_ptr(), rgb.data_ptr(), depth.data_ptr(), _lib.stream(dev))
    img = lambda x: x.reshape(1, H, W, -1).permute(0, 3, 1, 2)
    return dict(scene_rgb=scene["fine_rgb"], scene_dep=scene["fine_dep"], scene_nor=scene["fine_nor"],
                mask=img(mask.to(torch.float32)), object_rgb=img(object_rgb), shadow=img(shadow), rgb=img(rgb),
                depth=img(depth))


def _lights(model, obj, probe_positions, probe_size, shadows, shadow_probe, near, far, chunk_rays):
    dev = _model_device(model)
    if not isinstance(obj, VirtualObject):
        raise ValueError(f"obj must be a VirtualObject; got {type(obj).__name__}")
    if obj.device != dev:
        raise RuntimeError(f"the object is on {obj.device}, the model on {dev}")
    pos = _positions(obj, probe_positions, dev)
    probes = light_probes(model, pos, *probe_size, near=near, far=far, chunk_rays=chunk_rays)
    sprobe = None
    if shadows:
        sprobe = light_probes(model, obj.centroid(), *shadow_probe, near=near, far=far, chunk_rays=chunk_rays)
    return pos, probes, sprobe


def insert_object(model, camera, c2w, obj, probe_positions=None, probe_size=(32, 64), shadows=True, shadow_probe=(8, 16),
                  shadow_bias=1e-3, near=0.0, far=10.0, chunk_rays=32768, accel=None):
    """One view of the scene with `obj` in it -> dict of [1, C, H, W] fp32 tensors:

        scene_rgb, scene_dep, scene_nor   render_view's fine_rgb, fine_dep, fine_nor of the frame
        mask         1 where the object is hit in front of the scene (t < scene_dep; a NaN depth counts as behind)
        object_rgb   shade(...) at the hit pixels, 0 elsewhere; probes = light_probes(model, probe_positions, *probe_size)
        shadow       shadow_ratio at the scene's points outside the mask (1 inside, all 1 with shadows=False), from a
                     light_probes of size shadow_probe at the vertex centroid
        rgb          mask ? object_rgb : scene_rgb * shadow
        depth        mask ? t : scene_dep

    camera: views.perspective_camera(...) or views.pano_camera(h, w); the rays are the ones render_view renders.
    An object with texture maps gets the frame rays' radii in hit_attributes(radii=...) and, with a roughness_map,
    shade(roughness=the per-hit rows).  probe_positions [K, 3] (K <= 8) defaults to the vertex centroid; with K > 1 each hit blends the probes by the
    normalised inverse distances to their positions.  It is exactly light_probes -> trace_mesh -> hit_attributes ->
    shade / shadow_ratio(hit_attributes' scene_points, scene_nor) -> the composite, all public.  accel (None, "bvh" or a
    MeshBVH of the object) goes to trace_mesh and shadow_ratio; "bvh" is obj.bvh(), built once and kept on the object."""
    _check_accel(accel)
    camera, dev, _ = views._setup(model, camera, chunk_rays)
    pos, probes, sprobe = _lights(model, obj, probe_positions, probe_size, shadows, shadow_probe, near, far, chunk_rays)
    return _insert(model, camera, c2w, obj, pos, probes, sprobe, shadow_bias, near, far, chunk_rays,
                   obj.bvh() if accel == "bvh" else accel)


def insert_path(model, camera, poses, obj, probe_positions=None, probe_size=(32, 64), shadows=True, shadow_probe=(8, 16),
                shadow_bias=1e-3, near=0.0, far=10.0, exposure=0.0, kinds=("ldr", "mask"), out_dir=None,
                chunk_rays=32768, accel=None):
    """insert_object over poses ([n, 4, 4] or [n, 3, 4] c2ws): dict kind -> uint8 [n, H, W, 3] frames, "ldr" = to_frame of
    rgb, "mask" = the mask as 0 / 255, "depth" = to_frame of depth.  The probes are rendered once, not per frame: the
    object does not move, and neither is its BVH (accel as in insert_object: one build for all frames).  With out_dir the
    frames go to out_dir/<kind>/<i:05d>.png and the returned dict is empty."""
    _check_accel(accel)
    camera, dev, _ = views._setup(model, camera, chunk_rays)
    kinds = tuple(kinds)
    bad = [k for k in kinds if k not in ("ldr", "mask", "depth")]
    if bad or not kinds:
        raise ValueError(f"kinds must be a non-empty subset of ['depth', 'ldr', 'mask']; got {kinds!r}")
    c2ws = views._c2w_stack(poses)
    H, W = camera.h, camera.w
    pos, probes, sprobe = _lights(model, obj, probe_positions, probe_size, shadows, shadow_probe, near, far, chunk_rays)
    accel = obj.bvh() if accel == "bvh" else accel  # one MeshBVH for every frame
    sink = views._FrameSink(kinds, c2ws.shape[0], H, W, dev, out_dir)
    for i in range(sink.n):
        out = _insert(model, camera, c2ws[i], obj, pos, probes, sprobe, shadow_bias, near, far, chunk_rays, accel)
        for k in kinds:
            if k == "ldr":
                sink.put(k, i, views.to_frame(out["rgb"], "ldr", exposure=exposure))
            elif k == "depth":
                sink.put(k, i, views.to_frame(out["depth"], "depth", near, far))
            else:
                sink.put(k, i, (out["mask"][0, 0] * 255.0).to(torch.uint8)[..., None].expand(H, W, 3))
    return sink.frames
