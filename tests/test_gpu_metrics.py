"""The evaluation kernels (csrc/pn_metrics.hip) through pano_nerf_amd.metrics: the reference's values
(tests/golden/metrics_ext.npz), the host restatements on fp64 copies of a 512 x 1024 panorama, bit reproducibility,
in-place reads of render_image's strided views, a rendered panorama end to end, degenerate sizes and status codes."""
import math

import numpy as np
import pytest
import torch

from pano_nerf_amd import metrics
from test_gpu_full import dev, make_pano
from test_metrics_ext import SIZES, check_golden

pytestmark = pytest.mark.gpu


def rel_close(got, want, rtol, name):
    if math.isnan(want):
        assert math.isnan(got), (name, got, want)
    else:
        assert abs(got - want) <= rtol * max(abs(want), 1e-3), (name, got, want)


@pytest.mark.parametrize("h,w", SIZES)
def test_device_metrics_match_reference(golden, h, w):
    check_golden(golden("metrics_ext"), h, w, dev())


def seeded_panorama(h=512, w=1024, seed=5):
    """render_image-shaped outputs ([1, C, H, W] permuted views of [H*W, C] buffers) and contiguous ground truths."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=gen)
    nrm = lambda *s: torch.randn(*s, generator=gen)
    rgb = rnd(h * w, 3) * 2.5
    rgb[rnd(h * w, 3) < 0.03] *= 8.0  # past the ACES knee
    depth = rnd(h * w, 1) * 5 + 0.2
    normal = nrm(h * w, 3)
    albedo = rnd(h * w, 3)
    view = lambda x: x.to(dev()).view(1, h, w, -1).permute(0, 3, 1, 2)
    render = (None, view(rgb), None, view(depth), view(normal), view(albedo), None, None, None)
    chw = lambda x: x.view(1, h, w, -1).permute(0, 3, 1, 2).contiguous().to(dev())
    gt = dict(gt_hdr=chw((rgb * (1 + 0.2 * nrm(h * w, 3))).clamp_min(0)),
              gt_depth=chw(depth * torch.exp(0.2 * nrm(h * w, 1))),
              gt_normal=chw(2.0 * (normal + 0.4 * nrm(h * w, 3))),
              gt_albedo=chw((albedo + 0.05 * nrm(h * w, 3)).clamp(0, 1)),
              depth_mask=chw((rnd(h * w, 1) > 0.3).float()))
    return render, gt


def test_evaluate_panorama_512x1024_fp64_host_reproducible_and_strided():
    render, gt = seeded_panorama()
    got = metrics.evaluate_panorama(render, **gt)
    assert len(got) == 25
    host = metrics.evaluate_panorama(tuple(None if x is None else x.cpu().double() for x in render),
                                     **{k: v.cpu().double() for k, v in gt.items()})
    assert set(host) == set(got)
    off = {k: (got[k], host[k]) for k in got if not abs(got[k] - host[k]) <= 1e-6 * max(abs(host[k]), 1e-3)}
    assert not off, off
    again = metrics.evaluate_panorama(render, **gt)
    assert again == got, "two calls on the same inputs differ"
    contiguous = tuple(None if x is None else x.contiguous() for x in render)
    assert metrics.evaluate_panorama(contiguous, **gt) == got, "strided views and contiguous copies differ"


def test_rendered_panorama_end_to_end():
    import pano_nerf_amd as pn
    H, W, N = 16, 32, 16
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = (0.1, -0.2, 0.05)
    rays = pn.generate_pano_rays(H, W, c2w)
    env = pn.generate_lit_rays(10, pn.rays.pano_pixel_radius(rays))
    img_rays = pn.Rays(*[x.view(1, H, W, -1) for x in rays])
    render = pn.render_image(make_pano(N), img_rays, env, H, W)
    gen = torch.Generator(device="cpu").manual_seed(3)
    noisy = lambda x, s: (x.cpu() + s * torch.randn(x.shape, generator=gen)).contiguous().to(dev())
    gt = dict(gt_hdr=noisy(render[1], 0.05).abs(), gt_depth=noisy(render[3], 0.1).abs() + 0.1,
              gt_normal=noisy(render[4], 0.3), gt_albedo=noisy(render[5], 0.05).clamp(0, 1),
              depth_mask=(torch.rand(1, 1, H, W, generator=gen) > 0.2).float().to(dev()))
    got = pn.evaluate_panorama(render, **gt)
    host = pn.evaluate_panorama(tuple(None if x is None else x.cpu() for x in render),
                                **{k: v.cpu() for k, v in gt.items()})
    assert set(got) == set(host) and len(got) == 25
    for k in got:
        assert math.isfinite(got[k]), k
        rel_close(got[k], host[k], 1e-6, k)


@pytest.mark.parametrize("c,h,w", [(1, 1, 1), (3, 1, 1), (1, 1, 7), (3, 9, 1), (1, 6, 13)])
def test_degenerate_sizes_match_host(c, h, w):
    gen = torch.Generator(device="cpu").manual_seed(h * 100 + w + c)
    x, y = torch.rand(c, h, w, generator=gen) * 2, torch.rand(c, h, w, generator=gen) * 2
    for tx, ty in ((0, 0), (2, 1)):
        a = metrics._image_sums(x.to(dev()), y.to(dev()), tx, ty).cpu()
        b = metrics._image_sums(x, y, tx, ty)
        # exact up to the last bits of pow() (two math libraries) where the pair is tone-mapped
        assert torch.allclose(a, b, rtol=1e-9 if tx == 0 else 1e-6, atol=1e-12), (a, b)
    sa, ma = metrics._ssim_sums(x.to(dev()), y.to(dev()), 2, 1, want_map=True)
    sb, mb = metrics._ssim_sums(x, y, 2, 1, want_map=True)
    assert torch.allclose(sa.cpu(), sb, rtol=1e-6, atol=1e-9) and torch.allclose(ma.cpu().double(), mb, atol=1e-6)
    if c == 3:
        na, nb = metrics._normal_sums(x.to(dev()) - 1, y.to(dev()) - 1, 2).cpu(), metrics._normal_sums(x - 1, y - 1, 2)
        assert torch.allclose(na, nb, rtol=1e-6, atol=1e-9), (na, nb)
    da, db = metrics._depth_sums(x.to(dev()), y.to(dev())).cpu(), metrics._depth_sums(x, y)
    assert torch.allclose(da, db, rtol=1e-9, atol=1e-12), (da, db)


def test_bad_shapes_raise_from_status_codes():
    work = torch.empty(1 << 14, dtype=torch.float64, device=dev())
    two = torch.rand(2, 4, 4, device=dev())
    with pytest.raises(RuntimeError, match="bad shape"):
        metrics._image_sums(two, two, work=work)
    with pytest.raises(RuntimeError, match="bad shape"):
        metrics._ssim_sums(two, two, work=work)
    with pytest.raises(RuntimeError, match="bad shape"):
        metrics.calc_ws_ssim(torch.rand(3, 0, 4, device=dev()), torch.rand(3, 0, 4, device=dev()))
    x = torch.rand(3, 4, 4, device=dev())
    with pytest.raises(RuntimeError, match="unsupported"):
        metrics._image_sums(x, x, 0, 5, work=work)
    with pytest.raises(RuntimeError, match="unsupported"):
        metrics.ssim(x[None], x[None], window_size=7)
    torch.cuda.synchronize()
