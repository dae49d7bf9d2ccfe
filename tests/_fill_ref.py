"""numpy restatement of the "finishing warped frames" section of include/panonerf_hip.h: depth-aware push-pull hole
filling (pn_fill_holes) and blending of warped layers by weight (pn_warp_blend).  Written from the header, not from the
kernels.  Everything is fp32, one operation at a time, sums from their first term to the left, so a correct kernel gives
the same bits.  Audited by tests/test_fill_cpu.py; the reference of tests/test_gpu_fill.py."""
import numpy as np

F = np.float32


def level_sizes(H, W, levels=None):
    """[(H_0, W_0), ..., (H_L, W_L)]: up to 1 x 1, or `levels` levels above the frame"""
    out = [(int(H), int(W))]
    while out[-1] != (1, 1) and (levels is None or len(out) - 1 < levels):
        h, w = out[-1]
        out.append(((h + 1) >> 1, (w + 1) >> 1))
    return out


def _ordered_sum(terms, keep):
    """sum of terms[k] over keep[k], in order, starting from the first kept term (fp32)"""
    acc = np.zeros(np.broadcast(terms[0], keep[0]).shape, F)
    has = np.zeros(keep[0].shape, bool)
    for t, k in zip(terms, keep):
        acc = np.where(k, np.where(has, acc + t, t), acc).astype(F)
        has = has | k
    return acc


def _kept(zs, q):
    """the known entries on the farthest surface: zf q <= z_i"""
    zf = np.maximum.reduce(zs)
    lim = (zf * q).astype(F)
    return [(z > 0) & (lim <= z) for z in zs], zf > 0


def _pull(col, z, q):
    """level l from level l - 1: col [C, H, W], z [H, W] (0 unknown)"""
    C, H, W = col.shape
    h, w = (H + 1) >> 1, (W + 1) >> 1
    cp = np.zeros((C, 2 * h, 2 * w), F)
    zp = np.zeros((2 * h, 2 * w), F)
    cp[:, :H, :W], zp[:H, :W] = col, z
    kids = [(0, 0), (0, 1), (1, 0), (1, 1)]
    zs = [zp[dy::2, dx::2] for dy, dx in kids]
    keep, any_known = _kept(zs, q)
    cnt = sum(k.astype(np.int32) for k in keep).astype(F)
    with np.errstate(all="ignore"):
        nz = np.where(any_known, _ordered_sum(zs, keep) / cnt, F(0)).astype(F)
        nc = np.stack([np.where(any_known, _ordered_sum([cp[c, dy::2, dx::2] for dy, dx in kids], keep) / cnt, F(0))
                       for c in range(C)]).astype(F)
    return nc, nz


def _taps(n_fine, n_coarse, wrap):
    """(near, far) index arrays of the coordinates 0 .. n_fine - 1 in the level above"""
    v = np.arange(n_fine)
    near = np.where(v & 1, (v - 1) >> 1, v >> 1)
    far = np.where(v & 1, (v + 1) >> 1, (v >> 1) - 1)
    far = far % n_coarse if wrap else np.clip(far, 0, n_coarse - 1)
    assert (near >= 0).all() and (near < n_coarse).all()
    return near, far


def _push(col, z, ccol, cz, q, wrap, writable):
    """fill the unknown texels of a level (col, z) from the level above (ccol, cz); -> col, z, written"""
    C, H, W = col.shape
    yn, yf = _taps(H, cz.shape[0], False)
    xn, xf = _taps(W, cz.shape[1], wrap)
    taps = [(yn, xn, 9), (yn, xf, 3), (yf, xn, 3), (yf, xf, 1)]
    zs = [cz[np.ix_(ys, xs)] for ys, xs, _ in taps]
    ws = [np.full((H, W), wt, F) for _, _, wt in taps]
    keep, any_known = _kept(zs, q)
    write = (z == 0) & any_known & writable
    with np.errstate(all="ignore"):
        wsum = _ordered_sum(ws, keep)
        nz = (_ordered_sum([(w * v).astype(F) for w, v in zip(ws, zs)], keep) / wsum).astype(F)
        nc = np.stack([_ordered_sum([(w * ccol[c][np.ix_(ys, xs)]).astype(F) for w, (ys, xs, _) in zip(ws, taps)], keep) / wsum
                       for c in range(C)]).astype(F)
    return np.where(write, nc, col).astype(F), np.where(write, nz, z).astype(F), write


def fill_holes(image, depth=None, known=None, domain=None, wrap_x=False, depth_ratio=0.05, levels=None):
    """image [N, C, H, W] fp32, depth [N, H, W] or None, known [N, H, W] bool or None (all known), domain [H, W] bool or None
    -> (image, depth or None, filled [N, H, W] bool)"""
    image = np.asarray(image, F)
    N, C, H, W = image.shape
    q = F(1) - F(depth_ratio)
    sizes = level_sizes(H, W, levels)
    out_i = image.copy()
    out_d = None if depth is None else np.asarray(depth, F).copy()
    filled = np.zeros((N, H, W), bool)
    dom = np.ones((H, W), bool) if domain is None else np.asarray(domain, bool)
    for n in range(N):
        k = dom.copy() if known is None else (np.asarray(known[n], bool) & dom)
        if depth is None:
            z0 = np.where(k, F(1), F(0)).astype(F)
        else:
            d = np.asarray(depth[n], F)
            with np.errstate(invalid="ignore"):
                k = k & (d > 0) & (d < np.inf)
            z0 = np.where(k, d, F(0)).astype(F)
        cols, zs = [image[n]], [z0]
        for _ in sizes[1:]:
            c, z = _pull(cols[-1], zs[-1], q)
            cols.append(c)
            zs.append(z)
        for l in range(len(sizes) - 2, -1, -1):
            cols[l], zs[l], wrote = _push(cols[l], zs[l], cols[l + 1], zs[l + 1], q, wrap_x,
                                          dom if l == 0 else np.ones(zs[l].shape, bool))
            if l == 0:
                filled[n] = wrote
        out_i[n] = np.where(filled[n], cols[0], image[n])
        if out_d is not None:
            out_d[n] = np.where(filled[n], zs[0], out_d[n])
    return out_i, out_d, filled


def blend(images, depths, weights, depth_ratio=0.05, fill=0.0):
    """images [S, D, C, H, W], depths [S, D, H, W], weights [S, D] -> (image [D, C, H, W], depth [D, H, W], coverage [D, H, W])"""
    images, depths = np.asarray(images, F), np.asarray(depths, F)
    S, D, C, H, W = images.shape
    w = np.asarray(weights, np.float64)
    w = (np.repeat(w[:, None], D, 1) if w.ndim == 1 else w).astype(F)
    q = F(1) - F(depth_ratio)
    with np.errstate(all="ignore"):
        counts = (depths > 0) & (depths < np.inf)
        zn = np.where(counts, depths, F(np.inf)).min(0)
        keep = [counts[s] & ((depths[s] * q).astype(F) <= zn) for s in range(S)]
        kept = sum(k.astype(np.int32) for k in keep)
        ws = [np.broadcast_to(w[s][:, None, None], (D, H, W)).astype(F) for s in range(S)]
        wsum = _ordered_sum(ws, keep)
        zb = (_ordered_sum([(ws[s] * depths[s]).astype(F) for s in range(S)], keep) / wsum).astype(F)
        zc = _ordered_sum([depths[s] for s in range(S)], keep)  # with one layer kept: that layer
        dep = np.where(kept == 0, F(np.nan), np.where(kept == 1, zc, zb)).astype(F)
        img = np.empty((D, C, H, W), F)
        for c in range(C):
            vb = (_ordered_sum([(ws[s] * images[s, :, c]).astype(F) for s in range(S)], keep) / wsum).astype(F)
            vc = _ordered_sum([images[s, :, c] for s in range(S)], keep)
            img[:, c] = np.where(kept == 0, F(fill), np.where(kept == 1, vc, vb))
    return img, dep, (kept > 0).astype(F)


# ------------------------------------------------------------------------------------------------------ test scenes
SIZES = [(1, 1), (1, 2), (3, 5), (7, 10), (8, 16)]


def scene(H, W, density, seed=0, N=2, C=3):
    """random colours in [0, 1), depths in [1, 4), a known map of the given density with at least one known pixel in the
    first image; the second image may have none"""
    rng = np.random.default_rng(1000 * H + 10 * W + seed)
    img = rng.uniform(0, 1, (N, C, H, W)).astype(F)
    dep = rng.uniform(1, 4, (N, H, W)).astype(F)
    known = rng.uniform(0, 1, (N, H, W)) < density
    known[0, rng.integers(H), rng.integers(W)] = True
    return img, dep, known


def background_scene():
    """a 12 x 16 frame: background 0.25 at depth 4, a foreground block of colour 1 at depth 1, a hole band to its right"""
    img = np.full((1, 1, 12, 16), 0.25, F)
    dep = np.full((1, 12, 16), 4.0, F)
    img[0, 0, 3:9, 5:10], dep[0, 3:9, 5:10] = 1.0, 1.0
    known = np.ones((1, 12, 16), bool)
    known[0, 2:10, 10:13] = False
    return img, dep, known
