"""Relighting rendered views: virtual point and spot lights with omnidirectional shadow maps.

The model decomposes a scene into albedo, normals, depth and HDR radiance; this module puts a lamp into the room and
shows the picture with it switched on.  A light's shadow map is the model's own fine-level distance rendered from the
light's position (a small light probe that keeps the distance, not the colour); the per-pixel, per-light visibility and
shading is one kernel (``pn_relight.hip``).  Everything runs on the HIP device under ``torch.no_grad()`` on the current
stream; CPU tensors raise, there is no host fallback.  Nothing in ``views``, ``lighting`` or ``objects`` changes.

    PointLight(position, intensity, axis, inner_deg, outer_deg, r_min)   an omni light, or a spot with a smooth cone
    light_rows(lights)                          float32 [L, 16] numpy rows of pn_relight's light layout
    pack_lights(lights, device)                 those rows as a device tensor
    shadow_maps(model, lights_or_positions, ...)    [L, H, W] distance maps (kind "pano", or "cube": [L, 6 W, W])
    relight(rgb, depth, normals, albedo, rays, lights, maps, ...)   dict rgb / direct / visibility, shaped like the inputs
    light_visibility(points, lights, maps, normals=None, ...)       [M, L] visibility of every light at 3-D points
    relight_view(model, camera, c2w, lights, env_rays, ...)         render_view's dict plus relit_rgb, direct, visibility
    relight_path(model, camera, poses, lights, env_rays, ...)       dict kind -> frames (or PNG / EXR files)

Units and conventions (the formulas are stated in include/panonerf_hip.h): intensity is radiant intensity in the
scene's radiance units times length^2 - a light of intensity I at distance r facing a surface adds irradiance I / r^2,
and the surface shows albedo / pi of it.  ``ambient`` scales the whole captured image.  The bias defaults are
conventions chosen on an analytic room (tests/_relight_ref.py), not measurements of a trained scene."""
import math

import numpy as np
import torch

from . import _lib, views
from .cameras import _c2w_stack, _camera, cubemap_camera, pano_camera
from .geometry import _model_device
from .rays import CameraRig

LIGHT_FLOATS = 16  # PN_LIGHT_FLOATS
MAX_PCF = 7        # PN_RELIGHT_MAX_PCF
_MAP_KINDS = {"pano": 0, "cube": 2}  # PN_CAM_PANO, PN_CAM_CUBE
_PATH_KINDS = ("ldr", "hdr", "direct")
_BASES = ("fine_rgb", "surface_rgb")


class PointLight:
    """A point light at `position` with RGB radiant `intensity` (one number: white).  With `axis` it is a spot light
    along that direction: full strength within inner_deg of the axis, none beyond outer_deg, a smoothstep between
    (inner_deg < outer_deg <= 180, both required).  r_min keeps 1 / r^2 finite next to the light: distances below it
    shade as r_min.  Validated here, on the host."""

    __slots__ = ("position", "intensity", "axis", "inner_deg", "outer_deg", "r_min")

    def __init__(self, position, intensity, axis=None, inner_deg=None, outer_deg=None, r_min=0.05):
        p = np.asarray(position, dtype=np.float64).reshape(-1)
        if p.shape != (3,) or not np.isfinite(p).all():
            raise ValueError(f"position must be 3 finite numbers; got {position!r}")
        i = np.asarray(intensity, dtype=np.float64).reshape(-1)
        if i.shape == (1,):
            i = np.repeat(i, 3)
        if i.shape != (3,) or not np.isfinite(i).all() or (i < 0).any():
            raise ValueError(f"intensity must be one or three finite numbers >= 0; got {intensity!r}")
        rm = float(r_min)
        if not (rm >= 0.0 and math.isfinite(rm)):
            raise ValueError(f"r_min must be finite and >= 0; got {r_min!r}")
        if axis is None:
            if inner_deg is not None or outer_deg is not None:
                raise ValueError("inner_deg / outer_deg need an axis")
            a, inner, outer = None, None, None
        else:
            a = np.asarray(axis, dtype=np.float64).reshape(-1)
            if a.shape != (3,) or not np.isfinite(a).all() or not np.linalg.norm(a) > 0:
                raise ValueError(f"axis must be 3 finite numbers, not all zero; got {axis!r}")
            a = a / np.linalg.norm(a)
            if inner_deg is None or outer_deg is None:
                raise ValueError("a spot light needs inner_deg and outer_deg")
            inner, outer = float(inner_deg), float(outer_deg)
            if not (0.0 <= inner < outer <= 180.0):  # NaN fails
                raise ValueError(f"a spot light needs 0 <= inner_deg < outer_deg <= 180; got {inner_deg!r}, {outer_deg!r}")
        self.position, self.intensity, self.axis, self.inner_deg, self.outer_deg, self.r_min = p, i, a, inner, outer, rm

    def row(self):
        """float32 [16]: position, intensity, axis (zero: omni), cos_inner, cos_outer, r_min, four reserved zeros"""
        r = np.zeros(LIGHT_FLOATS, np.float64)
        r[0:3], r[3:6], r[11] = self.position, self.intensity, self.r_min
        if self.axis is not None:
            r[6:9] = self.axis
            r[9], r[10] = math.cos(math.radians(self.inner_deg)), math.cos(math.radians(self.outer_deg))
        out = r.astype(np.float32)
        if self.axis is not None and not out[9] > out[10]:
            raise ValueError("inner_deg and outer_deg are too close: their cosines coincide in fp32")
        return out

    def __repr__(self):
        spot = "" if self.axis is None else f", axis={self.axis.tolist()}, inner_deg={self.inner_deg}, outer_deg={self.outer_deg}"
        return f"PointLight({self.position.tolist()}, {self.intensity.tolist()}{spot}, r_min={self.r_min})"


def light_rows(lights):
    """float32 [L, 16] numpy: the rows pn_relight reads, of a sequence of PointLight (L = 0 allowed)"""
    if isinstance(lights, PointLight):
        lights = [lights]
    lights = list(lights)
    bad = [type(x).__name__ for x in lights if not isinstance(x, PointLight)]
    if bad:
        raise ValueError(f"lights must be PointLight objects; got {bad[0]}")
    return np.stack([x.row() for x in lights]) if lights else np.zeros((0, LIGHT_FLOATS), np.float32)


def _hip_device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("pano_nerf_amd.relight runs on a HIP device only (got %s); there is no CPU fallback" % dev)
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def pack_lights(lights, device):
    """[L, 16] fp32 device tensor of light_rows(lights)"""
    rows = light_rows(lights)
    return torch.from_numpy(rows).to(_hip_device(device))


def _lights(lights):
    """lights (PointLight objects, or pack_lights' rows) -> [L, 16] rows, checked on the host: the tensor as given, or the
    numpy rows still to be uploaded"""
    if isinstance(lights, (torch.Tensor, np.ndarray)):
        if lights.ndim != 2 or lights.shape[1] != LIGHT_FLOATS:
            raise ValueError(f"packed lights must be [L, {LIGHT_FLOATS}]; got {tuple(lights.shape)}")
        return lights if isinstance(lights, torch.Tensor) else np.ascontiguousarray(lights, dtype=np.float32)
    return light_rows(lights)


def _light_tensor(rows, dev):
    """_lights' rows -> contiguous [L, 16] fp32 on dev"""
    if isinstance(rows, np.ndarray):
        return torch.from_numpy(rows).to(dev)
    if rows.device != dev:
        raise RuntimeError(f"lights are on {rows.device}, the rows on {dev}")
    return rows.detach().to(torch.float32).contiguous()


def _on_device(t, what):
    if t.device.type != "cuda":
        raise RuntimeError("pano_nerf_amd.relight runs on a HIP device only (the %s is on %s); there is no CPU fallback"
                           % (what, t.device))


def _params(map_kind, ambient, normal_offset, bias_abs, bias_rel, bias_slope, pcf):
    """the scalars of pn_relight, checked on the host: (kind code, five floats, k)"""
    if map_kind not in _MAP_KINDS:
        raise ValueError(f"map_kind must be one of {sorted(_MAP_KINDS)}; got {map_kind!r}")
    vals = []
    for name, v in (("ambient", ambient), ("normal_offset", normal_offset), ("bias_abs", bias_abs), ("bias_rel", bias_rel),
                    ("bias_slope", bias_slope)):
        f = float(v)
        if not math.isfinite(f) or abs(f) > float(np.finfo(np.float32).max):  # the entry point takes fp32
            raise ValueError(f"{name} must be finite; got {v!r}")
        if name.startswith("bias") and f < 0.0:
            raise ValueError(f"{name} must be >= 0; got {v!r}")
        vals.append(f)
    k = int(pcf)
    if k != pcf or k < 1 or k > MAX_PCF or k % 2 == 0:
        raise ValueError(f"pcf must be an odd integer in [1, {MAX_PCF}]; got {pcf!r}")
    return _MAP_KINDS[map_kind], vals, k


def _maps(maps, L, kind):
    """maps [L, Hm, Wm] -> (contiguous fp32 tensor or None, Hm, Wm); with L = 0 maps may be None"""
    if maps is None or L == 0:
        if maps is None and L:
            raise ValueError(f"{L} lights need their shadow maps (shadow_maps(model, lights, ...))")
        return None, (12 if kind == "cube" else 2), 2
    if not isinstance(maps, torch.Tensor) or maps.dim() != 3:
        raise ValueError(f"maps must be a [L, Hm, Wm] tensor; got {getattr(maps, 'shape', type(maps))}")
    n, Hm, Wm = (int(s) for s in maps.shape)
    if n != L:
        raise ValueError(f"{L} lights but {n} shadow maps")
    if Hm < 2 or Wm < 2 or (kind == "cube" and Hm != 6 * Wm):
        raise ValueError(f"a {kind} shadow map is at least 2 x 2" + (" and 6 W x W" if kind == "cube" else "")
                         + f"; got {Hm} x {Wm}")
    return maps, Hm, Wm


def _call(org, drc, dep, nrm, alb, rgb, lights, maps, Hm, Wm, kind, vals, k, want_colour):
    """one pn_relight launch on contiguous fp32 rows -> (out, direct, visibility) row tensors (None where not wanted)"""
    dev = org.device
    R, L = int(org.shape[0]), int(lights.shape[0])
    with torch.no_grad(), torch.cuda.device(dev):
        out = torch.empty(R, 3, dtype=torch.float32, device=dev) if want_colour else None
        direct = torch.empty(R, 3, dtype=torch.float32, device=dev) if want_colour else None
        vis = torch.empty(R, L, dtype=torch.float32, device=dev)
        _lib.call("pn_relight", R, org.data_ptr(), drc.data_ptr(), dep.data_ptr(), _lib.ptr(nrm), _lib.ptr(alb),
                  _lib.ptr(rgb), L, _lib.ptr(lights if L else None), kind, Hm, Wm, _lib.ptr(maps), *vals, k, _lib.ptr(out),
                  _lib.ptr(direct), vis.data_ptr(), _lib.stream(dev))
    return out, direct, vis


def _rows(t, width, image):
    """[1, C, H, W] (image) or [R, C] / [R] rows -> contiguous fp32 [R, C] (or [R] for width 1 rows)"""
    x = t.detach()
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if image:
        return x[0].permute(1, 2, 0).reshape(-1, width).contiguous()
    return x.reshape(-1, width).contiguous()


def shadow_maps(model, lights_or_positions, height=64, width=128, kind="pano", near=0.0, far=10.0, chunk_rays=32768):
    """[L, H, W] fp32 distance maps, one per light: the fine-level distance of the model along the rays of an
    identity-rotation camera at the light's position - lighting.light_probes with the distance kept instead of the colour:
    the same rig, the same two levels, no density-gradient sweep, no light gather.  kind "pano": an equirectangular
    height x width map; kind "cube": cubemap_camera(width), [L, 6 width, width] (height is not used).  The rays of both
    cameras are unit vectors, so the values are Euclidean distances.  lights_or_positions: PointLight objects, their
    rows, or a [L, 3] device tensor of positions.  Each map equals render_view(model, camera, [I | p], outputs=("depth",))["fine_dep"]
    bit for bit.

    The distance is the EXPECTED termination distance of the ray (the weighted mean over the samples), not the first
    surface crossing: it is what render_view calls depth, so a pixel's own depth and the map agree on what "the surface"
    is, and a semi-transparent region gives a blurred edge, not a hole."""
    if kind not in _MAP_KINDS:
        raise ValueError(f"kind must be one of {sorted(_MAP_KINDS)}; got {kind!r}")
    camera = cubemap_camera(width) if kind == "cube" else pano_camera(height, width)
    H, W = camera.h, camera.w
    chunk = views._chunk_rays(chunk_rays)
    dev = _model_device(model)
    if dev.type != "cuda":
        raise RuntimeError("pano_nerf_amd.relight runs on a HIP device only (the model is on %s); there is no CPU "
                           "fallback" % dev)
    positions = lights_or_positions
    if not isinstance(positions, (torch.Tensor, np.ndarray)):
        positions = light_rows(positions)
    if positions.ndim == 2 and positions.shape[1] == LIGHT_FLOATS:  # light rows: the position comes first
        positions = positions[:, :3]
    if positions.ndim != 2 or positions.shape[1] != 3:
        raise ValueError(f"positions must be [L, 3]; got {tuple(positions.shape)}")
    if isinstance(positions, np.ndarray):
        positions = torch.from_numpy(np.ascontiguousarray(positions, dtype=np.float32)).to(dev)
    else:
        _on_device(positions, "positions")
        if positions.device != dev:
            raise RuntimeError(f"positions are on {positions.device}, the model on {dev}")
        positions = positions.detach().to(torch.float32)
    P = int(positions.shape[0])
    out = torch.empty(P * H * W, 1, dtype=torch.float32, device=dev)
    if P == 0:
        return out.view(0, H, W)
    with torch.no_grad(), torch.cuda.device(dev):
        rig = views._probe_rig(positions, camera, dev)
        views._render_rows(model, rig, 0, P * H * W, None, False, False, near, far, chunk, {"fine_dep": out}, streams=1)
    return out.view(P, H, W)


def relight(rgb, depth, normals, albedo, rays, lights, maps, map_kind="pano", ambient=1.0, normal_offset=0.02,
            bias_abs=0.01, bias_rel=0.02, bias_slope=2.0, pcf=3):
    """Light what a view shows with virtual lights: -> dict "rgb" (= ambient rgb + direct), "direct" (albedo / pi times the
    lights' irradiance, shadows included) and "visibility" (per light, in [0, 1]), shaped like the inputs.

    rgb, albedo, normals: [1, 3, H, W] (render_view's fine_rgb / surface_rgb, albedo, fine_nor) or [R, 3] rows; depth:
    [1, 1, H, W] or [R] / [R, 1], the distance t along each ray (fine_dep).  normals may be None (no cosine, no slope bias).
    rays: the Rays the pixels were rendered along (origins, directions: [R, 3]), or (camera, c2w) to generate them.
    lights: PointLight objects (or pack_lights' rows); maps: shadow_maps(model, lights, ...) of the same kind.
    Images give [1, 3, H, W], [1, 3, H, W], [1, L, H, W]; rows give [R, 3], [R, 3], [R, L].

    A pixel is in shadow where it lies farther from the light than the map's surface by more than
    bias_abs + bias_rel z + a slope term (bias_slope x the distance a texel spans on a surface tilted as this one is); the
    lookup starts normal_offset above the surface and averages pcf x pcf bilinear comparisons.  Pixels with no depth (0, NaN,
    Inf) or no normal keep ambient rgb.  Repeated calls give the same bits."""
    kind, vals, k = _params(map_kind, ambient, normal_offset, bias_abs, bias_rel, bias_slope, pcf)
    for name, t in (("rgb", rgb), ("depth", depth), ("albedo", albedo)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor; got {type(t).__name__}")
    image = rgb.dim() == 4
    if image:
        if rgb.shape[0] != 1 or rgb.shape[1] != 3:
            raise ValueError(f"an image is [1, 3, H, W]; got rgb {tuple(rgb.shape)}")
        H, W = int(rgb.shape[2]), int(rgb.shape[3])
        R = H * W
        want3, want1 = (1, 3, H, W), ((1, 1, H, W),)
    else:
        if rgb.dim() != 2 or rgb.shape[1] != 3:
            raise ValueError(f"rgb must be [1, 3, H, W] or [R, 3]; got {tuple(rgb.shape)}")
        R = int(rgb.shape[0])
        want3, want1 = (R, 3), ((R,), (R, 1))
    if tuple(albedo.shape) != want3:
        raise ValueError(f"albedo must be shaped like rgb {want3}; got {tuple(albedo.shape)}")
    if normals is not None and (not isinstance(normals, torch.Tensor) or tuple(normals.shape) != want3):
        raise ValueError(f"normals must be None or shaped like rgb {want3}; got {getattr(normals, 'shape', type(normals))}")
    if tuple(depth.shape) not in want1:
        raise ValueError(f"depth must be {' or '.join(str(s) for s in want1)}; got {tuple(depth.shape)}")
    lights = _lights(lights)
    L = len(lights)
    maps, Hm, Wm = _maps(maps, L, map_kind)
    given = isinstance(rays, tuple) and hasattr(rays, "origins")
    if not given and not (isinstance(rays, (tuple, list)) and len(rays) == 2):
        raise ValueError("rays must be a Rays tuple or (camera, c2w)")
    if not given:
        camera = _camera(rays[0])
        if image and (camera.h, camera.w) != (H, W):
            raise ValueError(f"the image is {H} x {W} but the camera is {camera.h} x {camera.w}")
        if not image and camera.h * camera.w != R:
            raise ValueError(f"{R} rows but the camera has {camera.h * camera.w} pixels")
    for name, t in (("rgb", rgb), ("depth", depth), ("albedo", albedo), ("normals", normals), ("maps", maps)):
        if t is not None:
            _on_device(t, name)
            if t.device != rgb.device:
                raise RuntimeError(f"{name} is on {t.device} but rgb on {rgb.device}")
    dev = rgb.device
    if given:
        org, drc = rays.origins, rays.directions
        for name, t in (("origins", org), ("directions", drc)):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (R, 3):
                raise ValueError(f"rays.{name} must be [{R}, 3]; got {getattr(t, 'shape', type(t))}")
            _on_device(t, "rays")
            if t.device != dev:
                raise RuntimeError(f"rays are on {t.device} but rgb on {dev}")
    else:
        rig = CameraRig(camera, _c2w_stack(rays[1], single=True), dev)
        with torch.cuda.device(dev):
            r = rig.sample(torch.arange(R, dtype=torch.int64, device=dev), 0.0, 1.0)[0]
        org, drc = r.origins, r.directions
    lt = _light_tensor(lights, dev)
    out, direct, vis = _call(_rows(org, 3, False), _rows(drc, 3, False),
                             _rows(depth, 1, image).reshape(-1), None if normals is None else _rows(normals, 3, image),
                             _rows(albedo, 3, image), _rows(rgb, 3, image), lt,
                             None if maps is None else maps.detach().to(torch.float32).contiguous(), Hm, Wm, kind, vals, k, True)
    if image:
        return {"rgb": out.view(1, H, W, 3).permute(0, 3, 1, 2), "direct": direct.view(1, H, W, 3).permute(0, 3, 1, 2),
                "visibility": vis.view(1, H, W, L).permute(0, 3, 1, 2)}
    return {"rgb": out, "direct": direct, "visibility": vis}


def light_visibility(points, lights, maps, normals=None, map_kind="pano", normal_offset=0.02, bias_abs=0.01, bias_rel=0.02,
                     bias_slope=2.0, pcf=3):
    """[M, L] fp32: the visibility of every light at points [M, 3] (relight's "visibility": the same kernel, with the points
    as ray origins, zero directions and depth 1).  With normals [M, 3] a light behind the surface gives 0 and the slope
    bias applies; without, only the shadow map decides."""
    kind, vals, k = _params(map_kind, 1.0, normal_offset, bias_abs, bias_rel, bias_slope, pcf)
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be an [M, 3] tensor; got {getattr(points, 'shape', type(points))}")
    if normals is not None and (not isinstance(normals, torch.Tensor) or tuple(normals.shape) != tuple(points.shape)):
        raise ValueError(f"normals must be None or [M, 3] like points; got {getattr(normals, 'shape', type(normals))}")
    lights = _lights(lights)
    L = len(lights)
    maps, Hm, Wm = _maps(maps, L, map_kind)
    for name, t in (("points", points), ("normals", normals), ("maps", maps)):
        if t is not None:
            _on_device(t, name)
            if t.device != points.device:
                raise RuntimeError(f"{name} is on {t.device} but points on {points.device}")
    dev = points.device
    M = int(points.shape[0])
    org = _rows(points, 3, False)
    _, _, vis = _call(org, torch.zeros_like(org), torch.ones(M, dtype=torch.float32, device=dev),
                      None if normals is None else _rows(normals, 3, False), None, None, _light_tensor(lights, dev),
                      None if maps is None else maps.detach().to(torch.float32).contiguous(), Hm, Wm, kind, vals, k, False)
    return vis


def _map_size(map_size):
    try:
        h, w = (int(v) for v in map_size)
    except (TypeError, ValueError):
        raise ValueError(f"map_size must be (height, width); got {map_size!r}") from None
    return h, w


def relight_view(model, camera, c2w, lights, env_rays=None, base="fine_rgb", maps=None, map_size=(64, 128),
                 map_kind="pano", near=0.0, far=10.0, chunk_rays=32768, **kw):
    """Render one view and relight it: one render_view for rgb, depth, normal and albedo (so a PanoMipNeRF and env_rays
    are needed, as for every surface output), shadow_maps of the lights unless maps are given, then relight.  -> render_view's
    dict plus "relit_rgb", "direct" [1, 3, H, W] and "visibility" [1, L, H, W].  base: "fine_rgb" relights the rendered
    radiance, "surface_rgb" the Lambertian re-rendering.  map_size = (height, width) of the maps (a cube takes width);
    **kw goes to relight (ambient, normal_offset, bias_abs, bias_rel, bias_slope, pcf)."""
    if base not in _BASES:
        raise ValueError(f"base must be one of {_BASES}; got {base!r}")
    _params(map_kind, *(kw.get(n, d) for n, d in (("ambient", 1.0), ("normal_offset", 0.02), ("bias_abs", 0.01),
                                                  ("bias_rel", 0.02), ("bias_slope", 2.0), ("pcf", 3))))
    h, w = _map_size(map_size)
    lights = _lights(lights)
    L = len(lights)
    outputs = ("rgb", "depth", "normal", "albedo") + (("surface",) if base == "surface_rgb" else ())
    view = views.render_view(model, camera, c2w, env_rays, outputs, near, far, chunk_rays)
    if maps is None and L:
        maps = shadow_maps(model, lights, h, w, map_kind, near, far, chunk_rays)
    res = relight(view[base], view["fine_dep"], view["fine_nor"], view["albedo"], (camera, c2w), lights, maps, map_kind, **kw)
    return {**view, "relit_rgb": res["rgb"], "direct": res["direct"], "visibility": res["visibility"]}


def relight_path(model, camera, poses, lights, env_rays=None, base="fine_rgb", maps=None, map_size=(64, 128),
                 map_kind="pano", kinds=("ldr",), near=0.0, far=10.0, exposure=0.0, out_dir=None, chunk_rays=32768, **kw):
    """relight_view along poses ([n, 4, 4] or [n, 3, 4] c2ws), the shadow maps rendered once: dict kind -> frames, made as
    render_path makes them: "ldr" uint8 [n, H, W, 3] = to_frame(relit_rgb, "ldr", exposure=exposure), "hdr" fp32
    [n, H, W, 3] = relit_rgb itself, "direct" uint8 = to_frame(direct, "ldr", exposure=exposure).  With out_dir, frames go
    to out_dir/<kind>/<i:05d>.png (hdr/<i:05d>.exr) as they complete and the returned dict is empty."""
    kinds = tuple(kinds)
    bad = [k for k in kinds if k not in _PATH_KINDS]
    if bad or not kinds:
        raise ValueError(f"kinds must be a non-empty subset of {sorted(_PATH_KINDS)}; got {kinds!r}")
    camera = _camera(camera)
    c2ws = _c2w_stack(poses)
    h, w = _map_size(map_size)
    lights = _lights(lights)
    L = len(lights)
    dev = _model_device(model)
    if maps is None and L:
        maps = shadow_maps(model, lights, h, w, map_kind, near, far, chunk_rays)
    sink = views._FrameSink(kinds, c2ws.shape[0], camera.h, camera.w, dev, out_dir)
    lt = _light_tensor(lights, dev)  # uploaded once for every frame
    for i in range(sink.n):
        v = relight_view(model, camera, c2ws[i], lt, env_rays, base, maps, (h, w), map_kind, near, far, chunk_rays, **kw)
        for k in kinds:
            if k == "hdr":
                sink.put(k, i, v["relit_rgb"][0].permute(1, 2, 0))
            else:
                sink.put(k, i, views.to_frame(v["relit_rgb" if k == "ldr" else "direct"], "ldr", exposure=exposure))
    return sink.frames
