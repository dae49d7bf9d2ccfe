"""The light sources of a captured scene as editable lights: connected bright regions of HDR light probes.

``lighting`` renders probes and integrates them, ``ibl`` bakes them, ``relight`` adds new lamps; this module says where the
lamps of the captured room ARE and how strong they are.  A probe's emitter pixels (luminance above a threshold) are
segmented into connected components on the wrapped equirectangular grid, every component gets a radiometric record, and
with the model's distance along the same rays the record becomes a point light in ``relight``'s units.  The segmentation
and the records are HIP kernels (``pn_emitters.hip``); everything runs on the HIP device under ``torch.no_grad()`` on the
current stream; CPU tensors raise, there is no host fallback.  Nothing in ``lighting``, ``relight`` or ``views`` changes.

    probe_rgbd(model, positions, ...)             (probes [P, 3, H, W], distance [P, H, W]) from one pass of the model
    emitter_threshold(probes, ratio=8)            [P] the default threshold of each probe
    label_emitters(probes, threshold)             (labels int32 [P, H, W], count int32 [P])
    emitter_stats(probes, labels, count, distance=None)   dict of [P, Cmax, ...] records
    emitters_from_probes(probes, positions, ...)  per probe a list of Emitter records, brightest first
    extract_emitters(model, positions, size, ...) probe_rgbd then emitters_from_probes; also the probes, distances, labels
    residual_probes(probes, labels, distance=None, grow=0)   the environment with the emitters taken out (views.fill_holes)
    to_point_lights(emitters, standoff=0, r_min=None)        relight.PointLight objects
    save_lights(path, emitters) / load_lights(path)          one JSON file laid out like glTF's KHR_lights_punctual

Conventions (stated term for term in include/panonerf_hip.h, discussed in DESIGN.md 6j): luminance is the channel mean;
a pixel is an emitter when its luminance is strictly above the threshold; the default threshold is ``ratio`` times the
solid-angle-weighted geometric mean luminance - the rule and ratio = 8 are conventions, not measurements; components are
8-connected with the left and right image borders joined and are numbered by their smallest pixel index.  Intensity is
radiant intensity in the scene's radiance units times length^2, as in ``relight``: not candela."""
import json
import math

import numpy as np
import torch

from . import _lib, views
from .cameras import pano_camera
from .geometry import _model_device
from .lighting import _cuda, _probe_view, _table
from .relight import PointLight

_FIELDS = ("pixels", "omega", "flux", "lum_flux", "direction", "peak", "peak_index", "spread", "angular_radius", "distance")
UNITS = ("intensity is radiant intensity in the scene's radiance units times scene length^2 (a light of intensity I at "
         "distance r adds irradiance I / r^2); it is not candela")


class Emitter:
    """One connected bright region of one probe and the point light it stands for.  The record (pixels, omega, flux [3],
    lum_flux, direction [3], peak, peak_index, spread, angular_radius, distance) is emitter_stats' row; probe and label say
    where it came from; position = probe position + direction x distance, radius = distance x sin(min(angular_radius,
    pi / 2)) and intensity [3] = flux x distance^2 are NaN without a distance."""

    __slots__ = ("probe", "label") + _FIELDS + ("position", "radius", "intensity")

    def __init__(self, probe, label, record, probe_position):
        self.probe, self.label = int(probe), int(label)
        for k in _FIELDS:
            v = record[k]
            setattr(self, k, int(v) if k in ("pixels", "peak_index") else (np.asarray(v, np.float64) if np.ndim(v) else float(v)))
        d = self.distance
        self.position = np.asarray(probe_position, np.float64) + self.direction * d
        self.radius = d * math.sin(min(self.angular_radius, 0.5 * math.pi))
        self.intensity = self.flux * (d * d)

    def __repr__(self):
        return (f"Emitter(probe={self.probe}, label={self.label}, pixels={self.pixels}, lum_flux={self.lum_flux:.6g}, "
                f"direction={self.direction.tolist()}, distance={self.distance:.6g}, position={self.position.tolist()})")


def probe_rgbd(model, positions, height=64, width=128, near=0.0, far=10.0, chunk_rays=32768):
    """(probes [P, 3, H, W], distance [P, H, W]) fp32 from ONE pass of the model: bit for bit lighting.light_probes and
    relight.shadow_maps(kind="pano") of the same arguments - they run the same rig and keep the fine level's radiance and
    its distance respectively.  probes is a view of a contiguous [P, H, W, 3] buffer, as light_probes returns it."""
    P = views._probe_positions(positions)
    camera = pano_camera(height, width)
    H, W = camera.h, camera.w
    dev = _cuda(positions)
    if _model_device(model) != dev:
        raise RuntimeError(f"positions are on {dev}, the model on {_model_device(model)}")
    chunk = views._chunk_rays(chunk_rays)
    rgb = torch.empty(P * H * W, 3, dtype=torch.float32, device=dev)
    dist = torch.empty(P * H * W, 1, dtype=torch.float32, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        rig = views._probe_rig(positions, camera, dev)
        views._render_rows(model, rig, 0, P * H * W, None, False, False, near, far, chunk,
                           {"fine_rgb": rgb, "fine_dep": dist}, streams=1)
    return rgb.view(P, H, W, 3).permute(0, 3, 1, 2), dist.view(P, H, W)


def emitter_threshold(probes, ratio=8.0):
    """[P] fp32: ratio x exp(sum omega ln max(Y, 1e-6) / sum omega) over the pixels of each probe with a finite luminance
    Y - ratio times the solid-angle-weighted geometric mean (the arithmetic mean is dominated by the lamps themselves).
    A convention, as is ratio = 8."""
    r = float(ratio)
    if not (r > 0.0 and math.isfinite(r)):
        raise ValueError(f"ratio must be finite and positive; got {ratio!r}")
    x, sp, sc, sw, P, H, W = _probe_view(probes)
    dev = x.device
    with torch.no_grad(), torch.cuda.device(dev):
        _, omega = _table(H, W, dev)
        out = torch.empty(P, dtype=torch.float32, device=dev)
        _lib.call("pn_emitter_threshold", P, H, W, x.data_ptr(), sp, sc, sw, omega.data_ptr(), r, out.data_ptr(),
                  _lib.stream(dev))
    return out


def _threshold(threshold, P, dev):
    if isinstance(threshold, torch.Tensor):
        if tuple(threshold.shape) != (P,):
            raise ValueError(f"threshold must be a number or a [{P}] tensor, one value per probe; got {tuple(threshold.shape)}")
        _cuda(threshold)
        if threshold.device != dev:
            raise RuntimeError(f"threshold is on {threshold.device} but the probes on {dev}")
        return threshold.detach().to(torch.float32).contiguous()
    try:
        t = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"threshold must be a number or a [{P}] tensor; got {threshold!r}") from None
    return torch.full((P,), t, dtype=torch.float32, device=dev)


def label_emitters(probes, threshold):
    """(labels int32 [P, H, W], count int32 [P]): the connected components of the pixels whose luminance is strictly above
    threshold (a number, rounded to fp32, or [P]: one per probe) under the 8-neighbourhood with the left and right borders joined (rows 0
    and H - 1 are not joined across the poles).  -1 is background; a probe's components are numbered 0 .. count - 1 in
    ascending order of their smallest row-major pixel index.  A NaN pixel is no emitter, a +inf pixel is one.  No host
    synchronisation; repeated calls give the same bits."""
    x, sp, sc, sw, P, H, W = _probe_view(probes)
    dev = x.device
    thr = _threshold(threshold, P, dev)
    with torch.no_grad(), torch.cuda.device(dev):
        parent = torch.empty(P, H * W, dtype=torch.int32, device=dev)
        labels = torch.empty(P, H, W, dtype=torch.int32, device=dev)
        flags = torch.empty(P, H * W, dtype=torch.int32, device=dev)
        count = torch.empty(P, dtype=torch.int32, device=dev)
        st = _lib.stream(dev)
        _lib.call("pn_emitter_labels", P, H, W, x.data_ptr(), sp, sc, sw, thr.data_ptr(), parent.data_ptr(), labels.data_ptr(),
                  flags.data_ptr(), st)
        prefix = torch.cumsum(flags, 1, dtype=torch.int32)  # roots are numbered by a prefix count, as pn_bvh uses torch.sort
        _lib.call("pn_emitter_compact", P, H, W, prefix.data_ptr(), labels.data_ptr(), count.data_ptr(), st)
    return labels, count


def _labels(labels, count, P, H, W, dev):
    if not isinstance(labels, torch.Tensor) or tuple(labels.shape) != (P, H, W) or labels.dtype != torch.int32:
        raise ValueError(f"labels must be an int32 [P, H, W] = {(P, H, W)} tensor matching the probes; got "
                         f"{getattr(labels, 'dtype', type(labels))} {getattr(labels, 'shape', '')}")
    _cuda(labels)
    if labels.device != dev:
        raise RuntimeError(f"labels are on {labels.device} but the probes on {dev}")
    if count is not None:
        if not isinstance(count, torch.Tensor) or tuple(count.shape) != (P,) or count.dtype != torch.int32:
            raise ValueError(f"count must be an int32 [{P}] tensor; got {getattr(count, 'dtype', type(count))} "
                             f"{getattr(count, 'shape', '')}")
        _cuda(count)
        if count.device != dev:
            raise RuntimeError(f"count is on {count.device} but the probes on {dev}")
    return labels.detach().contiguous()


def _distance(distance, P, H, W, dev):
    if distance is None:
        return None
    if not isinstance(distance, torch.Tensor) or tuple(distance.shape) not in ((P, H, W), (P, 1, H, W)):
        raise ValueError(f"distance must be [P, H, W] = {(P, H, W)} or [P, 1, H, W]; got {getattr(distance, 'shape', type(distance))}")
    _cuda(distance)
    if distance.device != dev:
        raise RuntimeError(f"distance is on {distance.device} but the probes on {dev}")
    return distance.detach().to(torch.float32).reshape(P, H, W).contiguous()


def emitter_stats(probes, labels, count, distance=None):
    """The record of every component: dict of [P, Cmax, ...] device tensors - pixels (int32), omega, flux [.., 3], lum_flux,
    direction [.., 3], peak, peak_index (int32), spread, angular_radius, distance (fp32) - as include/panonerf_hip.h states
    them; fp64 sums in a fixed order, the same bits on every call.  Cmax = int(count.max()) is the one host
    synchronisation.  Rows beyond a probe's count are zero, with pixels = 0.  distance: the model's distance along the
    probe's rays ([P, H, W], probe_rgbd's), or None: the records' distance is NaN.

    The pixels are grouped by component with one stable torch.sort and each component is summed by one wave, so the cost
    follows the number of pixels and of components, not their product."""
    x, sp, sc, sw, P, H, W = _probe_view(probes)
    dev = x.device
    lab = _labels(labels, count, P, H, W, dev)
    z = _distance(distance, P, H, W, dev)
    HW = H * W
    with torch.no_grad(), torch.cuda.device(dev):
        C = int(count.max())
        if C < 0 or C > HW:
            raise ValueError(f"count holds {C}: not a component count of a {H} x {W} probe")
        S = P * C
        f = lambda *s: torch.zeros(P, C, *s, dtype=torch.float32, device=dev)
        i = lambda: torch.zeros(P, C, dtype=torch.int32, device=dev)
        out = dict(pixels=i(), omega=f(), flux=f(3), lum_flux=f(), direction=f(3), peak=f(), peak_index=i(), spread=f(),
                   angular_radius=f(), distance=f())
        if C == 0:
            return out
        dirs, omega = _table(H, W, dev)
        lab = lab.view(P, HW).to(torch.int64)
        key = torch.where((lab >= 0) & (lab < C), lab + torch.arange(P, device=dev).view(P, 1) * C, S).view(-1)
        skey, order = torch.sort(key, stable=True)  # background (key S) last; pixel order kept within a component
        starts = torch.searchsorted(skey, torch.arange(S + 1, dtype=torch.int64, device=dev))
        N = P * HW
        _lib.call("pn_emitter_stats", P, H, W, x.data_ptr(), sp, sc, sw, dirs.data_ptr(), omega.data_ptr(), _lib.ptr(z), C, N,
                  order.data_ptr(), starts.data_ptr(), *(out[k].data_ptr() for k in _FIELDS), _lib.stream(dev))
    return out


def _positions(positions, P):
    p = positions.detach().cpu().numpy() if isinstance(positions, torch.Tensor) else np.asarray(positions)
    if p.shape != (P, 3):
        raise ValueError(f"positions must be [P, 3] = {(P, 3)}, one per probe; got {p.shape}")
    return p.astype(np.float64)


def _extract(probes, positions, distance, threshold, ratio, min_solid_angle, max_emitters):
    m, cap = float(min_solid_angle), int(max_emitters)
    if not m >= 0.0:
        raise ValueError(f"min_solid_angle must be >= 0; got {min_solid_angle!r}")
    if cap != max_emitters or cap < 0:
        raise ValueError(f"max_emitters must be a non-negative integer; got {max_emitters!r}")
    _probe_view(probes)
    pos = _positions(positions, int(probes.shape[0]))
    thr = emitter_threshold(probes, ratio) if threshold is None else threshold
    labels, count = label_emitters(probes, thr)
    rec = {k: v.cpu().numpy() for k, v in emitter_stats(probes, labels, count, distance).items()}
    cnt = count.cpu().numpy()
    lists = []
    for p in range(len(cnt)):
        es = [Emitter(p, c, {k: rec[k][p, c] for k in _FIELDS}, pos[p]) for c in range(int(cnt[p]))]
        es = [e for e in es if e.omega >= m]
        es.sort(key=lambda e: (-e.lum_flux, e.label))
        lists.append(es[:cap])
    return lists, labels, count


def emitters_from_probes(probes, positions, distance=None, threshold=None, ratio=8.0, min_solid_angle=0.0, max_emitters=16):
    """Per probe a list of Emitter records, sorted by descending lum_flux (ties by label): the model-free core.  probes
    [P, 3, H, W] on the device, positions [P, 3] (tensor or array) of the probes, distance [P, H, W] or None (then the
    lights have no position: distance, position, radius and intensity are NaN).  threshold: a number or [P]; None: the
    default, emitter_threshold(probes, ratio).  Components whose solid angle is under min_solid_angle are dropped; each
    list is cut at max_emitters."""
    return _extract(probes, positions, distance, threshold, ratio, min_solid_angle, max_emitters)[0]


def extract_emitters(model, positions, size=(64, 128), near=0.0, far=10.0, chunk_rays=32768, threshold=None, ratio=8.0,
                     min_solid_angle=0.0, max_emitters=16):
    """Exactly probe_rgbd(model, positions, *size, near, far, chunk_rays) followed by emitters_from_probes: dict "emitters"
    (per probe a list of Emitter), "probes" [P, 3, H, W], "distance" [P, H, W], "labels" int32 [P, H, W] and "count" [P]."""
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (height, width); got {size!r}") from None
    probes, dist = probe_rgbd(model, positions, h, w, near, far, chunk_rays)
    lists, labels, count = _extract(probes, positions, dist, threshold, ratio, min_solid_angle, max_emitters)
    return {"emitters": lists, "probes": probes, "distance": dist, "labels": labels, "count": count}


def residual_probes(probes, labels, distance=None, grow=0):
    """The environment with the emitters taken out: [P, 3, H, W], bit for bit
    views.fill_holes(probes, distance, labels < 0, pano_camera(H, W))["image"] - the background-preferring, seam-wrapping
    hole filler, with the emitter pixels as the holes.  grow dilates the removed set by that many pixels first
    (8-neighbourhood, columns wrapped; plain torch on the device), to take a lamp's halo with it.  Pixels that stay keep
    their bits.  A residual probe goes through ibl.bake_ibl / ibl.save_ibl unchanged."""
    x, _, _, _, P, H, W = _probe_view(probes)
    lab = _labels(labels, None, P, H, W, x.device)
    g = int(grow)
    if g != grow or g < 0:
        raise ValueError(f"grow must be a non-negative integer; got {grow!r}")
    with torch.no_grad(), torch.cuda.device(x.device):
        known = lab < 0
        if g:
            gone = (~known).to(torch.float32).view(P, 1, H, W)
            for _ in range(g):
                wrapped = torch.cat([gone[..., -1:], gone, gone[..., :1]], -1)
                gone = torch.nn.functional.max_pool2d(wrapped, 3, stride=1, padding=(1, 0))
            known = gone.view(P, H, W) == 0
    return views.fill_holes(probes, distance, known, pano_camera(H, W))["image"]


def _flat(emitters):
    if isinstance(emitters, Emitter):
        return [emitters]
    out = []
    for e in emitters:
        out.extend(_flat(e) if not isinstance(e, Emitter) else [e])
    return out


def to_point_lights(emitters, standoff=0.0, r_min=None):
    """relight.PointLight objects of Emitter records (a list, or emitters_from_probes' list of lists, flattened in order).
    standoff moves each light that far back towards its probe, so that a shadow map rendered from it does not start inside
    the lamp's own geometry; r_min defaults to the emitter's radius.  An emitter without a finite distance raises,
    named."""
    s = float(standoff)
    if not (s >= 0.0 and math.isfinite(s)):
        raise ValueError(f"standoff must be finite and >= 0; got {standoff!r}")
    lights = []
    for e in _flat(emitters):
        if not (math.isfinite(e.distance) and e.distance > 0.0):
            raise ValueError(f"emitter {e.label} of probe {e.probe} has no distance ({e.distance}): extract it with a distance "
                             "map (probe_rgbd, extract_emitters) before turning it into a light")
        lights.append(PointLight(e.position - e.direction * s, e.intensity, r_min=e.radius if r_min is None else r_min))
    return lights


def save_lights(path, emitters):
    """One JSON file, one entry per light, laid out like glTF's KHR_lights_punctual: type "point", color (the intensity
    normalised to its largest channel), intensity (that channel), position, radius, direction (from the probe), solid_angle,
    and the probe it came from.  The units are the scene's (UNITS), not candela; the file says so."""
    lights = []
    for e in _flat(emitters):
        top = float(np.max(e.intensity))
        if not math.isfinite(top):
            raise ValueError(f"emitter {e.label} of probe {e.probe} has no finite intensity (distance {e.distance})")
        color = (e.intensity / top).tolist() if top > 0.0 else [1.0, 1.0, 1.0]
        lights.append({"name": f"probe{e.probe}_emitter{e.label}", "type": "point", "color": color, "intensity": top,
                       "position": e.position.tolist(), "radius": float(e.radius), "direction": e.direction.tolist(),
                       "solid_angle": float(e.omega), "probe": e.probe})
    doc = {"asset": {"generator": "pano_nerf_amd.emitters", "layout": "KHR_lights_punctual", "units": UNITS},
           "lights": lights}
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)


def load_lights(path):
    """relight.PointLight objects of a save_lights file: position, color x intensity, r_min = radius."""
    with open(path) as fh:
        doc = json.load(fh)
    out = []
    for i, e in enumerate(doc.get("lights", [])):
        if e.get("type") != "point":
            raise ValueError(f"light {i} of {path} is of type {e.get('type')!r}; only point lights are written here")
        out.append(PointLight(e["position"], np.asarray(e["color"], np.float64) * float(e["intensity"]), r_min=e["radius"]))
    return out
