// pn_emitters.hip — the light sources of an HDR light probe as objects (gfx950): the default emitter threshold of a probe,
// connected-component labelling of its bright pixels on the wrapped equirectangular grid, and the radiometric record of
// every component.  The conventions (luminance, emitter pixel, adjacency, label order, the record's fields) are stated in
// include/panonerf_hip.h.
//
// Every floating-point sum runs in fp64 on the fp32 inputs in an order that depends on the shapes only (a lane walks its
// elements in index order, the lanes meet in a fixed butterfly) and every output is rounded once; the only atomics are
// 32-bit integer atomicMin on the parent array of the union-find, whose RESULT (the smallest pixel index of a component)
// does not depend on the order in which they land.  Two calls on the same inputs give the same bits.  Radiance is read in
// place through the (probe, channel, pixel) strides of pn_probes.h's Probes.
#include "pn_common.h"
#include "pn_probes.h"
#include "pn_unionfind.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / PN_WAVE;
constexpr int kThrThreads = 1024;  // the threshold's single workgroup per probe: as wide as a workgroup gets
constexpr int kThrWaves = kThrThreads / PN_WAVE;

// Y = ((double)R + G + B) / 3.0 of pixel pix of the probe at xp
__device__ __forceinline__ double luminance(const float* xp, const Probes& pr, int64_t pix) {
    const double r = xp[pix * pr.ps], g = xp[pr.cs + pix * pr.ps], b = xp[2 * pr.cs + pix * pr.ps];
    return ((r + g) + b) / 3.0;
}

// ---- 1. the default threshold: ratio exp(sum omega ln max(Y, 1e-6) / sum omega) over the pixels with finite Y ------------
// One workgroup of 1024 threads per probe.  Thread t adds pixels t, t + 1024, ... in that order, a wave adds its lanes in
// the butterfly and thread 0 adds the sixteen waves in order: the tree's shape is a function of H W alone.
__global__ __launch_bounds__(kThrThreads) void k_emitter_threshold(int64_t HW, Probes pr, const float* omega, double ratio,
                                                                  float* out) {
    const int64_t p = blockIdx.x;
    const float* xp = pr.x + p * pr.probe_stride;
    double num = 0.0, den = 0.0;
    for (int64_t pix = threadIdx.x; pix < HW; pix += kThrThreads) {
        const double y = luminance(xp, pr, pix);
        if (isfinite(y)) {
            const double w = omega[pix];
            num += w * log(y > 1e-6 ? y : 1e-6);
            den += w;
        }
    }
    __shared__ double red[2][kThrWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    num = wave_sum(num);
    den = wave_sum(den);
    if (lane == 0) red[0][wv] = num, red[1][wv] = den;
    __syncthreads();
    if (threadIdx.x == 0) {
        double n = red[0][0], d = red[1][0];
        for (int w = 1; w < kThrWaves; ++w) n += red[0][w], d += red[1][w];
        out[p] = (float)(ratio * exp(n / d));  // no finite pixel: 0 / 0, a NaN threshold, under which nothing is an emitter
    }
}

// ---- 2. labelling: union-find over pixel indices --------------------------------------------------------------------
// parent[p HW + i] is an index within probe p, or -1 for a pixel that is no emitter.  INVARIANT (P1): a stored value is
// never larger than its own index: k_emitter_init stores i itself, and the only later writer is atomicMin(&parent[a], b)
// with b < a, which can only lower it.  So parent[i] <= i at every moment, for every reader, however stale its copy.

__global__ __launch_bounds__(kThreads) void k_emitter_init(int64_t P, int64_t HW, Probes pr, const float* threshold,
                                                          int32_t* parent) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= P * HW) return;
    const int64_t p = e / HW, pix = e % HW;
    const double y = luminance(pr.x + p * pr.probe_stride, pr, pix);
    parent[e] = y > (double)threshold[p] ? (int32_t)pix : -1;  // strict; a NaN on either side compares false
}

// load_parent / find_root / unite: pn_unionfind.h (shared with pn_meshops.hip), with the termination argument

// every emitter pixel (i, j) unites with the emitters among (i, j - 1), (i - 1, j - 1), (i - 1, j), (i - 1, j + 1), columns
// modulo W: each adjacent pair of the wrapped 8-neighbourhood exactly once (twice where W = 2 makes j - 1 and j + 1 one
// column, which is harmless); rows are not joined across a pole
__global__ __launch_bounds__(kThreads) void k_emitter_union(int64_t P, int H, int W, int32_t* parent) {
    const int64_t HW = (int64_t)H * W;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= P * HW) return;
    int32_t* par = parent + (e / HW) * HW;
    const int32_t pix = (int32_t)(e % HW);
    if (load_parent(par, pix) < 0) return;
    const int i = pix / W, j = pix % W;
    const int jm = j == 0 ? W - 1 : j - 1, jp = j == W - 1 ? 0 : j + 1;
    const int32_t nb[4] = {i * W + jm, (i - 1) * W + jm, (i - 1) * W + j, (i - 1) * W + jp};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q > 0 && i == 0) break;
        if (load_parent(par, nb[q]) >= 0) unite(par, pix, nb[q]);
    }
}

// roots[e] = the root of pixel e (-1: no emitter), flags[e] = 1 at a root.  parent is only read here.
__global__ __launch_bounds__(kThreads) void k_emitter_flatten(int64_t P, int64_t HW, const int32_t* parent, int32_t* roots,
                                                             int32_t* flags) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= P * HW) return;
    const int32_t* par = parent + (e / HW) * HW;
    int32_t i = (int32_t)(e % HW);
    const int32_t self = i;
    int32_t q = par[i];
    if (q >= 0) {
        while (q != i) {  // (P1) again: strictly down to the root
            i = q;
            q = par[i];
        }
    }
    roots[e] = q;
    flags[e] = q == self ? 1 : 0;
}

// labels[e]: on entry the root of pixel e, on exit the rank of that root among the roots of its probe (prefix = the
// inclusive count of flags along each probe).  A thread reads and writes its own element of labels only.
__global__ __launch_bounds__(kThreads) void k_emitter_compact(int64_t P, int64_t HW, const int32_t* prefix, int32_t* labels,
                                                             int32_t* count) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= P * HW) return;
    const int64_t p = e / HW;
    const int32_t r = labels[e];
    labels[e] = (r >= 0 && r < HW) ? prefix[p * HW + r] - 1 : -1;
    if (e % HW == HW - 1) count[p] = prefix[e];
}

// ---- 3. the record of every component ------------------------------------------------------------------------------
struct StatsArgs {
    int64_t HW;
    Probes pr;
    const float *dirs, *omega, *distance;
    int64_t S, N;
    int Cmax;
    const int64_t *order, *starts;
    int32_t* pixels;
    float *omega_out, *flux, *lum_flux, *direction, *peak;
    int32_t* peak_index;
    float *spread, *angular_radius, *dist_out;
};

// One wave per segment s = p Cmax + c: order[starts[s] .. starts[s + 1]) are the pixels (p HW + pix) of component c of
// probe p in ascending order.  Lane l takes elements l, l + 64, ... in order; the lanes meet in the xor butterfly.  The
// work is one visit (two for the spread) of every emitter pixel plus one wave per segment: it does not grow as C x HW.
__global__ __launch_bounds__(kThreads) void k_emitter_stats(StatsArgs a) {
    const int64_t s = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (s >= a.S) return;
    const int lane = threadIdx.x & 63;
    int64_t lo = a.starts[s], hi = a.starts[s + 1];
    lo = lo < 0 ? 0 : (lo > a.N ? a.N : lo);
    hi = hi < lo ? lo : (hi > a.N ? a.N : hi);
    if (hi == lo) return;  // rows beyond a probe's count stay as the caller zeroed them
    const int64_t p = s / a.Cmax;
    const float* xp = a.pr.x + p * a.pr.probe_stride;
    const float* dist = a.distance ? a.distance + p * a.HW : nullptr;
    double n = 0.0, om = 0.0, f0 = 0.0, f1 = 0.0, f2 = 0.0, lum = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, dn = 0.0, dd = 0.0,
           dc = 0.0;
    double py = -(double)INFINITY;
    int32_t pi = 0x7fffffff;
    for (int64_t k = lo + lane; k < hi; k += 64) {
        const int64_t pix = a.order[k] - p * a.HW;
        if (pix < 0 || pix >= a.HW) continue;  // not a pixel of this probe: a malformed order is skipped, never read
        const double w = a.omega[pix];
        const double r = xp[pix * a.pr.ps], g = xp[a.pr.cs + pix * a.pr.ps], b = xp[2 * a.pr.cs + pix * a.pr.ps];
        const double y = ((r + g) + b) / 3.0;
        const double yw = y * w;
        n += 1.0;
        om += w;
        f0 += r * w, f1 += g * w, f2 += b * w;
        lum += yw;
        s0 += yw * (double)a.dirs[pix * 3], s1 += yw * (double)a.dirs[pix * 3 + 1], s2 += yw * (double)a.dirs[pix * 3 + 2];
        if (dist) {
            const float z = dist[pix];
            if (z > 0.f && z < INFINITY) dn += yw * (double)z, dd += yw, dc += 1.0;
        }
        if (y > py || (y == py && (int32_t)pix < pi)) py = y, pi = (int32_t)pix;
    }
    n = wave_sum(n), om = wave_sum(om), f0 = wave_sum(f0), f1 = wave_sum(f1), f2 = wave_sum(f2), lum = wave_sum(lum);
    s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2), dn = wave_sum(dn), dd = wave_sum(dd), dc = wave_sum(dc);
    for (int o = 32; o > 0; o >>= 1) {
        const double oy = __shfl_xor(py, o, 64);
        const int32_t oi = __shfl_xor(pi, o, 64);
        if (oy > py || (oy == py && oi < pi)) py = oy, pi = oi;
    }
    if (n == 0.0) return;
    if (pi < 0 || pi >= a.HW) pi = 0;  // unreachable with n > 0 and luminances that are not NaN; keeps the read below in bounds
    // the flux-weighted mean direction, or the peak pixel's where the weighted directions cancel (or are not finite)
    const double norm = sqrt((s0 * s0 + s1 * s1) + s2 * s2);
    double d0, d1, d2;
    if (norm > 0.0 && norm < (double)INFINITY && norm >= 1e-12 * lum) {
        d0 = s0 / norm, d1 = s1 / norm, d2 = s2 / norm;
    } else {
        d0 = a.dirs[(int64_t)pi * 3], d1 = a.dirs[(int64_t)pi * 3 + 1], d2 = a.dirs[(int64_t)pi * 3 + 2];
    }
    // spread: the largest angle atan2(|d x u|, d . u) between the direction and a pixel's
    double sp = 0.0;
    for (int64_t k = lo + lane; k < hi; k += 64) {
        const int64_t pix = a.order[k] - p * a.HW;
        if (pix < 0 || pix >= a.HW) continue;
        const double u0 = a.dirs[pix * 3], u1 = a.dirs[pix * 3 + 1], u2 = a.dirs[pix * 3 + 2];
        const double c0 = d1 * u2 - d2 * u1, c1 = d2 * u0 - d0 * u2, c2 = d0 * u1 - d1 * u0;
        const double ang = atan2(sqrt((c0 * c0 + c1 * c1) + c2 * c2), (d0 * u0 + d1 * u1) + d2 * u2);
        sp = ang > sp ? ang : sp;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_xor(sp, o, 64);
        sp = os > sp ? os : sp;
    }
    if (lane != 0) return;
    a.pixels[s] = (int32_t)n;
    a.omega_out[s] = (float)om;
    a.flux[s * 3] = (float)f0, a.flux[s * 3 + 1] = (float)f1, a.flux[s * 3 + 2] = (float)f2;
    a.lum_flux[s] = (float)lum;
    a.direction[s * 3] = (float)d0, a.direction[s * 3 + 1] = (float)d1, a.direction[s * 3 + 2] = (float)d2;
    a.peak[s] = (float)py;
    a.peak_index[s] = pi;
    a.spread[s] = (float)sp;
    const double cap = om < 4.0 * kPiD ? om : 4.0 * kPiD;
    a.angular_radius[s] = (float)acos(1.0 - cap / (2.0 * kPiD));
    a.dist_out[s] = dc > 0.0 ? (float)(dn / dd) : NAN;
}

// P < 2^25 probes of H x W < 2^30 pixels (pn_lighting's bounds), H and W >= 2, and P H W < 2^39 so that ceil(P H W / 256)
// workgroups fit a grid
int check_probes(int64_t P, int H, int W) {
    if (P <= 0 || H < 2 || W < 2 || P >= (1 << 25) || (int64_t)H * W >= ((int64_t)1 << 30)) return PN_ERR_BAD_SHAPE;
    if (P * ((int64_t)H * W) >= ((int64_t)1 << 39)) return PN_ERR_BAD_SHAPE;
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_emitter_threshold(int64_t P, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps,
                         const float* omega, double ratio, float* threshold, void* stream) {
    int st = check_probes(P, H, W);
    if (st != PN_OK) return st;
    if (!(isfinite(ratio) && ratio > 0.0)) return PN_ERR_BAD_SHAPE;
    if (!x || !omega || !threshold) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_emitter_threshold, dim3((unsigned)P), dim3(kThrThreads), 0, ST(stream), (int64_t)H * W,
                       Probes{x, probe_stride, cs, ps}, omega, ratio, threshold);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_emitter_labels(int64_t P, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps,
                      const float* threshold, int32_t* parent, int32_t* roots, int32_t* flags, void* stream) {
    int st = check_probes(P, H, W);
    if (st != PN_OK) return st;
    if (!x || !threshold || !parent || !roots || !flags) return PN_ERR_NULL;
    const int64_t HW = (int64_t)H * W;
    const dim3 grid(nblk(P * HW, kThreads)), block(kThreads);
    hipLaunchKernelGGL(k_emitter_init, grid, block, 0, ST(stream), P, HW, Probes{x, probe_stride, cs, ps}, threshold, parent);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_emitter_union, grid, block, 0, ST(stream), P, H, W, parent);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_emitter_flatten, grid, block, 0, ST(stream), P, HW, parent, roots, flags);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_emitter_compact(int64_t P, int H, int W, const int32_t* prefix, int32_t* labels, int32_t* count, void* stream) {
    int st = check_probes(P, H, W);
    if (st != PN_OK) return st;
    if (!prefix || !labels || !count) return PN_ERR_NULL;
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(k_emitter_compact, dim3(nblk(P * HW, kThreads)), dim3(kThreads), 0, ST(stream), P, HW, prefix, labels,
                       count);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_emitter_stats(int64_t P, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps,
                     const float* dirs, const float* omega, const float* distance, int Cmax, int64_t N,
                     const int64_t* order, const int64_t* starts, int32_t* pixels, float* omega_out, float* flux,
                     float* lum_flux, float* direction, float* peak, int32_t* peak_index, float* spread,
                     float* angular_radius, float* distance_out, void* stream) {
    int st = check_probes(P, H, W);
    if (st != PN_OK) return st;
    const int64_t HW = (int64_t)H * W;
    if (Cmax < 0 || (int64_t)Cmax > HW || N < 0 || N > P * HW) return PN_ERR_BAD_SHAPE;
    if (Cmax == 0) return PN_OK;
    if (!x || !dirs || !omega || !starts || (N > 0 && !order)) return PN_ERR_NULL;
    if (!pixels || !omega_out || !flux || !lum_flux || !direction || !peak || !peak_index || !spread || !angular_radius ||
        !distance_out)
        return PN_ERR_NULL;
    const int64_t S = P * Cmax;
    if ((int64_t)nblk(S, kWaves) >= ((int64_t)1 << 31)) return PN_ERR_BAD_SHAPE;
    StatsArgs a{HW,     Probes{x, probe_stride, cs, ps}, dirs, omega, distance, S,          N,     Cmax,
                order,  starts,                          pixels, omega_out, flux, lum_flux, direction, peak,
                peak_index, spread, angular_radius, distance_out};
    hipLaunchKernelGGL(k_emitter_stats, dim3(nblk(S, kWaves)), dim3(kThreads), 0, ST(stream), a);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
