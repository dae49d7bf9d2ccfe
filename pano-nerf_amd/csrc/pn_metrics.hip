// pn_metrics.hip — evaluation of a rendered H x W equirectangular panorama (gfx950): image error sums with optional
// tone mapping, SSIM (11 x 11 Gaussian window, zero padding), normal angle / cosine sums and the depth metrics of
// utils/metrics.py.  Every kernel is a reduction: a fixed grid, one row of fp64 partial sums per workgroup in the
// caller's workspace, then one workgroup that sums the rows in a fixed order (no atomics: two calls on the same inputs
// give the same bits).  Per-element arithmetic is fp64 except where the reference's result depends on an fp32 rounding:
// the tone mapping (its uint8 truncation) and the cosine of F.cosine_similarity (its overshoot past +-1).
//
// Operands are read in place through (channel stride, pixel stride) pairs: element (c, i, j) of a [C, H, W] image is
// p[c * cs + (i * W + j) * ps], which covers contiguous [C, H, W] tensors (cs = H*W, ps = 1) and the [1, C, H, W]
// permuted views of [H*W, C] buffers that render_image returns (cs = 1, ps = C).
#include "pn_common.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;  // grid cap of the element-wise reductions (grid-stride beyond it)
constexpr int kTileW = 32, kTileH = 16, kRad = 5, kWin = 2 * kRad + 1;
constexpr int kStageW = kTileW + 2 * kRad, kStageH = kTileH + 2 * kRad;
constexpr int kSumsQ = 6, kSsimQ = 3, kNormQ = 5, kDepthQ = 9;

struct Img {
    const float* p;
    int64_t cs, ps;
    int tone;  // 0 none, 1 hdr_to_ldr float, 2 hdr_to_ldr uint8
};

inline unsigned elem_grid(int64_t n) {
    unsigned g = nblk(n, kThreads);
    return g < (unsigned)kMaxBlocks ? g : (unsigned)kMaxBlocks;
}

// clamp01 and tonemap (hdr_to_ldr) live in pn_common.h: pn_views.hip's LDR frames use the same arithmetic

__device__ __forceinline__ float load(const Img& m, int c, int64_t pix) { return tonemap(m.p[c * m.cs + pix * m.ps], m.tone); }

// normalised solid-angle weight of a pixel in row i: sin((i + 1/2) pi / H) / (W * sum_i sin(...)); the row sum is
// 1 / sin(pi / 2H) in closed form
__device__ __forceinline__ double pixel_weight(int i, int H, int W) {
    return sin((i + 0.5) * M_PI / H) * sin(M_PI / (2.0 * H)) / W;
}

// sum v[] over the workgroup (fixed butterfly, then the four waves in order) and store it at dst[0..NQ)
template <int NQ>
__device__ __forceinline__ void block_store(double (&v)[NQ], double* dst) {
    __shared__ double red[NQ][kThreads / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double s = wave_sum(v[q]);
        if (lane == 0) red[q][wv] = s;
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        double s = red[threadIdx.x][0];
        for (int w = 1; w < kThreads / 64; ++w) s += red[threadIdx.x][w];
        dst[threadIdx.x] = s;
    }
}

// out[q] = sum over the nb partial rows, in a fixed order
template <int NQ>
__global__ __launch_bounds__(kThreads) void k_finish(const double* part, int nb, double* out) {
    double v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = 0.0;
    for (int b = threadIdx.x; b < nb; b += kThreads)
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] += part[(int64_t)b * NQ + q];
    block_store<NQ>(v, out);
}

// [sum d^2, sum |d|, sum w d^2, sum w |d|, sum d, count], d = tonemap(x) - tonemap(y)
__global__ __launch_bounds__(kThreads) void k_sums(int C, int H, int W, Img x, Img y, double* part) {
    double v[kSumsQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t P = (int64_t)H * W;
    int row = -1;
    double w = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < P; p += (int64_t)gridDim.x * kThreads) {
        const int i = (int)(p / W);
        if (i != row) row = i, w = pixel_weight(i, H, W);
        for (int c = 0; c < C; ++c) {
            const double d = (double)load(x, c, p) - (double)load(y, c, p);
            const double d2 = d * d, ad = fabs(d);
            v[0] += d2;
            v[1] += ad;
            v[2] += w * d2;
            v[3] += w * ad;
            v[4] += d;
            v[5] += 1.0;
        }
    }
    block_store<kSumsQ>(v, part + (int64_t)blockIdx.x * kSumsQ);
}

// SSIM over one kTileH x kTileW tile of one channel (utils/metrics.py:44-200 with F.conv2d(padding=5)): the tile and
// a 5-pixel halo of both tone-mapped images go to LDS (zeros outside the image), a horizontal 11-tap pass writes the
// five moments of every staged row, a vertical pass finishes them per output pixel.  -> [sum s, sum w s, count]
__global__ __launch_bounds__(kThreads) void k_ssim(int C, int H, int W, Img x, Img y, const double* taps, double c1,
                                                   double c2, float* map, double* part) {
    __shared__ float sx[kStageH][kStageW + 1], sy[kStageH][kStageW + 1];
    __shared__ double hs[5][kStageH][kTileW];
    double g[kWin];
#pragma unroll
    for (int u = 0; u < kWin; ++u) g[u] = taps[u];
    const int c = blockIdx.z, i0 = blockIdx.y * kTileH, j0 = blockIdx.x * kTileW;
    for (int k = threadIdx.x; k < kStageH * kStageW; k += kThreads) {
        const int r = k / kStageW, q = k % kStageW, i = i0 + r - kRad, j = j0 + q - kRad;
        const bool in = i >= 0 && i < H && j >= 0 && j < W;
        const int64_t pix = (int64_t)i * W + j;
        sx[r][q] = in ? load(x, c, pix) : 0.f;
        sy[r][q] = in ? load(y, c, pix) : 0.f;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kStageH * kTileW; k += kThreads) {
        const int r = k / kTileW, q = k % kTileW;
        double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
        for (int u = 0; u < kWin; ++u) {
            const double a = sx[r][q + u], b = sy[r][q + u];
            mx += g[u] * a;
            my += g[u] * b;
            xx += g[u] * (a * a);
            yy += g[u] * (b * b);
            xy += g[u] * (a * b);
        }
        hs[0][r][q] = mx, hs[1][r][q] = my, hs[2][r][q] = xx, hs[3][r][q] = yy, hs[4][r][q] = xy;
    }
    __syncthreads();
    double v[kSsimQ] = {0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < kTileH * kTileW; k += kThreads) {
        const int r = k / kTileW, q = k % kTileW, i = i0 + r, j = j0 + q;
        if (i >= H || j >= W) continue;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < kWin; ++u)
#pragma unroll
            for (int e = 0; e < 5; ++e) m[e] += g[u] * hs[e][r + u][q];
        const double m11 = m[0] * m[0], m22 = m[1] * m[1], m12 = m[0] * m[1];
        const double s11 = m[2] - m11, s22 = m[3] - m22, s12 = m[4] - m12;
        const double s = ((2.0 * m12 + c1) * (2.0 * s12 + c2)) / ((m11 + m22 + c1) * (s11 + s22 + c2));
        if (map) map[((int64_t)c * H + i) * W + j] = (float)s;
        v[0] += s;
        v[1] += pixel_weight(i, H, W) * s;
        v[2] += 1.0;
    }
    const int64_t b = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    block_store<kSsimQ>(v, part + b * kSsimQ);
}

// ||v|| as ATen's linalg_vector_norm evaluates three fp32 components (fused multiply-adds in index order)
__device__ __forceinline__ float norm3(float a, float b, float c) { return sqrtf(fmaf(c, c, fmaf(b, b, a * a))); }

// [sum angle, sum w angle, sum cos, sum w cos, count]: cos = F.cosine_similarity(x, y) over the 3 channels, bit for bit
// (each vector divided by max(||v||, 1e-8), products summed in order); angle = nan_to_num(acos(cos)) in degrees, so a
// cosine that rounds past +-1 scores 0 degrees as in the reference.  y is first put through `y_normalize` passes of
// F.normalize (v / max(||v||, 1e-12)).
__global__ __launch_bounds__(kThreads) void k_normals(int H, int W, Img x, Img y, int y_normalize, double* part) {
    double v[kNormQ] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t P = (int64_t)H * W;
    int row = -1;
    double w = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < P; p += (int64_t)gridDim.x * kThreads) {
        const int i = (int)(p / W);
        if (i != row) row = i, w = pixel_weight(i, H, W);
        float a[3], b[3];
        for (int c = 0; c < 3; ++c) a[c] = x.p[c * x.cs + p * x.ps], b[c] = y.p[c * y.cs + p * y.ps];
        for (int k = 0; k < y_normalize; ++k) {
            float n = norm3(b[0], b[1], b[2]);
            n = n < 1e-12f ? 1e-12f : n;  // clamp_min: NaN stays NaN
            for (int c = 0; c < 3; ++c) b[c] = b[c] / n;
        }
        float na = norm3(a[0], a[1], a[2]), nb = norm3(b[0], b[1], b[2]);
        na = na < 1e-8f ? 1e-8f : na;
        nb = nb < 1e-8f ? 1e-8f : nb;
        const float cs = ((a[0] / na) * (b[0] / nb) + (a[1] / na) * (b[1] / nb)) + (a[2] / na) * (b[2] / nb);
        double ang = acos((double)cs) * (180.0 / M_PI);
        if (isnan(ang)) ang = 0.0;
        v[0] += ang;
        v[1] += w * ang;
        v[2] += cs;
        v[3] += w * cs;
        v[4] += 1.0;
    }
    block_store<kNormQ>(v, part + (int64_t)blockIdx.x * kNormQ);
}

// utils/metrics.py:290-315 over the elements with mask > 0 (all of them if mask is null):
// [count, sum |d|/g, sum d^2/g, sum d^2, log count, sum (log p - log g)^2, delta_1, delta_2, delta_3 counts];
// the log terms also need p > 1e-7 and g > 1e-7 (fp32 comparisons, as torch makes them), and delta_k counts
// max(p/g, g/p) < 1.25^k with torch.max's NaN propagation (a NaN ratio is never an inlier)
__global__ __launch_bounds__(kThreads) void k_depth(int64_t n, const float* pred, int64_t p_st, const float* gt,
                                                    int64_t g_st, const float* mask, int64_t m_st, double* part) {
    double v[kDepthQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
        if (mask && !(mask[e * m_st] > 0.f)) continue;
        const float pf = pred[e * p_st], gf = gt[e * g_st];
        const double p = pf, g = gf, d = p - g, d2 = d * d;
        v[0] += 1.0;
        v[1] += fabs(d) / g;
        v[2] += d2 / g;
        v[3] += d2;
        if (pf > 1e-7f && gf > 1e-7f) {
            const double l = log(p) - log(g);
            v[4] += 1.0;
            v[5] += l * l;
        }
        const double r1 = p / g, r2 = g / p;
        v[6] += (r1 < 1.25 && r2 < 1.25) ? 1.0 : 0.0;
        v[7] += (r1 < 1.5625 && r2 < 1.5625) ? 1.0 : 0.0;
        v[8] += (r1 < 1.953125 && r2 < 1.953125) ? 1.0 : 0.0;
    }
    block_store<kDepthQ>(v, part + (int64_t)blockIdx.x * kDepthQ);
}

int check_image(int C, int H, int W, int tx, int ty) {
    if (H <= 0 || W <= 0 || (C != 1 && C != 3)) return PN_ERR_BAD_SHAPE;
    if (tx < 0 || tx > 2 || ty < 0 || ty > 2) return PN_ERR_UNSUPPORTED;
    return PN_OK;
}

}  // namespace

extern "C" {

int64_t pn_metrics_work_doubles(int C, int H, int W) {
    if (check_image(C, H, W, 0, 0) != PN_OK) return PN_ERR_BAD_SHAPE;
    const int64_t tiles = (int64_t)nblk(W, kTileW) * nblk(H, kTileH) * C;
    const int64_t elem = (int64_t)kMaxBlocks * kDepthQ;
    return tiles * kSsimQ > elem ? tiles * kSsimQ : elem;
}

int pn_metric_sums(int C, int H, int W, const float* x, int64_t x_cs, int64_t x_ps, int x_tone, const float* y,
                   int64_t y_cs, int64_t y_ps, int y_tone, double* out, double* work, void* stream) {
    int st = check_image(C, H, W, x_tone, y_tone);
    if (st != PN_OK) return st;
    if (!x || !y || !out || !work) return PN_ERR_NULL;
    const unsigned nb = elem_grid((int64_t)H * W);
    hipLaunchKernelGGL(k_sums, dim3(nb), dim3(kThreads), 0, ST(stream), C, H, W, Img{x, x_cs, x_ps, x_tone},
                       Img{y, y_cs, y_ps, y_tone}, work);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_finish<kSumsQ>, dim3(1), dim3(kThreads), 0, ST(stream), work, (int)nb, out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_metric_ssim(int C, int H, int W, const float* x, int64_t x_cs, int64_t x_ps, int x_tone, const float* y,
                   int64_t y_cs, int64_t y_ps, int y_tone, int window, const double* taps, double max_val, float* map,
                   double* out, double* work, void* stream) {
    int st = check_image(C, H, W, x_tone, y_tone);
    if (st != PN_OK) return st;
    if (window != kWin) return PN_ERR_UNSUPPORTED;
    if (!x || !y || !taps || !out || !work) return PN_ERR_NULL;
    const double c1 = (0.01 * max_val) * (0.01 * max_val), c2 = (0.03 * max_val) * (0.03 * max_val);
    const dim3 grid(nblk(W, kTileW), nblk(H, kTileH), C);
    hipLaunchKernelGGL(k_ssim, grid, dim3(kThreads), 0, ST(stream), C, H, W, Img{x, x_cs, x_ps, x_tone},
                       Img{y, y_cs, y_ps, y_tone}, taps, c1, c2, map, work);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_finish<kSsimQ>, dim3(1), dim3(kThreads), 0, ST(stream), work, (int)(grid.x * grid.y * grid.z),
                       out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_metric_normals(int H, int W, const float* x, int64_t x_cs, int64_t x_ps, const float* y, int64_t y_cs,
                      int64_t y_ps, int y_normalize, double* out, double* work, void* stream) {
    if (H <= 0 || W <= 0) return PN_ERR_BAD_SHAPE;
    if (y_normalize < 0 || y_normalize > 2) return PN_ERR_UNSUPPORTED;
    if (!x || !y || !out || !work) return PN_ERR_NULL;
    const unsigned nb = elem_grid((int64_t)H * W);
    hipLaunchKernelGGL(k_normals, dim3(nb), dim3(kThreads), 0, ST(stream), H, W, Img{x, x_cs, x_ps, 0},
                       Img{y, y_cs, y_ps, 0}, y_normalize, work);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_finish<kNormQ>, dim3(1), dim3(kThreads), 0, ST(stream), work, (int)nb, out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_metric_depth(int64_t n, const float* pred, int64_t pred_st, const float* gt, int64_t gt_st, const float* mask,
                    int64_t mask_st, double* out, double* work, void* stream) {
    if (n <= 0) return PN_ERR_BAD_SHAPE;
    if (!pred || !gt || !out || !work) return PN_ERR_NULL;
    const unsigned nb = elem_grid(n);
    hipLaunchKernelGGL(k_depth, dim3(nb), dim3(kThreads), 0, ST(stream), n, pred, pred_st, gt, gt_st, mask, mask_st,
                       work);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_finish<kDepthQ>, dim3(1), dim3(kThreads), 0, ST(stream), work, (int)nb, out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
