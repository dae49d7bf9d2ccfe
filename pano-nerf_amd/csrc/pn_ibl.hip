// pn_ibl.hip — light probes baked into the image-based-lighting assets engines consume (gfx950): the GGX-prefiltered
// radiance of a probe around a direction (split sum, N = V = R; Karis, "Real Shading in Unreal Engine 4"), the
// two-channel environment-BRDF table, and the engine's evaluation of both with an irradiance cube.  Formulas and
// conventions are stated in include/panonerf_hip.h.
//
// Every sum runs in fp64 in a fixed order on fp32 inputs and is rounded once per output.  The prefilter is a quadrature
// over every probe pixel, not Monte Carlo: a workgroup takes 256 directions of one probe, one per thread, and one
// segment of the probe's pixels, staged through LDS in tiles of 256 (pn_lighting.hip's k_probe_irradiance); the
// segments' partial sums go to the caller's workspace and a second launch adds them in order (the pn_probe_sh
// pattern).  The number of segments is a function of the pixel count only, so a probe's result does not depend on P.
// No atomics: two calls on the same inputs give the same bits.  Radiance is read in place through (probe, channel,
// pixel) strides.
//
// NaN, as in pn_probe_irradiance: a NaN radiance value makes that channel NaN for EVERY direction of its probe, those
// facing away from the pixel included (weight 0 times NaN), and a NaN dot product stays NaN.
#include "pn_common.h"
#include "pn_probes.h"
#include "pn_rays.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 256;     // pixels staged per LDS tile
constexpr int kSegTiles = 4;   // tiles one pixel segment covers at least
constexpr int kMaxSegs = 64;   // pixel segments per probe at most
constexpr int kMaxLut = 4096;  // largest table size and node count per axis

// pixel segments of a probe: `segs` runs of `tiles` LDS tiles each (the last one shorter), from the pixel count alone
struct Split {
    int segs, tiles;
};
inline Split split_of(int64_t hw) {
    const int64_t nt = (hw + kTile - 1) / kTile;
    int64_t want = (nt + kSegTiles - 1) / kSegTiles;
    if (want > kMaxSegs) want = kMaxSegs;
    const int64_t per = (nt + want - 1) / want;
    return Split{(int)((nt + per - 1) / per), (int)per};
}

// workgroup g = (p * nkb + b) * nseg + s: directions b * 256 .. b * 256 + 255 of probe p over the pixels of segment s.
// Per pixel c = relu(n . d), h2 = (1 + c) / 2, den = h2 (alpha^2 - 1) + 1, q = c / den^2;
// part[((p K + n) nseg + s) 4 + (0..2)] = sum (L_ch omega) q, [+ 3] = sum omega q  (L omega is exact in fp64)
__global__ __launch_bounds__(kThreads) void k_prefilter(int64_t HW, int64_t K, int nkb, int nseg, int seg_tiles, Probes pr,
                                                       const float* dirs, const float* omega, const float* normals,
                                                       int64_t normal_stride, double a2m1, double* part) {
    __shared__ double4 s_dir[kTile], s_rad[kTile];  // (d, omega), (L omega, -)
    const int s = (int)(blockIdx.x % nseg);
    const int64_t g = blockIdx.x / nseg;
    const int64_t p = g / nkb;
    const int64_t n = (g % nkb) * kThreads + threadIdx.x;
    const float* xp = pr.x + p * pr.probe_stride;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (n < K) {
        const float* np_ = normals + p * normal_stride + n * 3;
        nx = np_[0], ny = np_[1], nz = np_[2];
    }
    const int64_t first = (int64_t)s * seg_tiles * kTile;
    const int64_t last = first + (int64_t)seg_tiles * kTile < HW ? first + (int64_t)seg_tiles * kTile : HW;
    double e0 = 0.0, e1 = 0.0, e2 = 0.0, ew = 0.0;
    for (int64_t base = first; base < last; base += kTile) {
        const int cnt = (int)((last - base) < kTile ? (last - base) : kTile);
        for (int t = threadIdx.x; t < cnt; t += kThreads) {
            const int64_t pix = base + t;
            const double w = omega[pix];
            s_dir[t] = make_double4(dirs[pix * 3], dirs[pix * 3 + 1], dirs[pix * 3 + 2], w);
            s_rad[t] = make_double4((double)xp[pix * pr.ps] * w, (double)xp[pr.cs + pix * pr.ps] * w,
                                    (double)xp[2 * pr.cs + pix * pr.ps] * w, 0.0);
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const double4 d = s_dir[t];
            double c = nx * d.x + ny * d.y + nz * d.z;
            c = c < 0.0 ? 0.0 : c;  // relu as torch evaluates it: NaN stays NaN
            const double den = ((1.0 + c) / 2.0) * a2m1 + 1.0;
            const double q = c / (den * den);
            const double4 r = s_rad[t];
            e0 += r.x * q;
            e1 += r.y * q;
            e2 += r.z * q;
            ew += d.w * q;
        }
        __syncthreads();
    }
    if (n < K) {
        double* o = part + ((p * K + n) * nseg + s) * 4;
        o[0] = e0, o[1] = e1, o[2] = e2, o[3] = ew;
    }
}

// out[p, n, ch] = (sum_s part[.., s, ch]) / (sum_s part[.., s, 3]), segments in order
__global__ __launch_bounds__(kThreads) void k_prefilter_finish(int64_t PK, int nseg, const double* part, float* out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= PK) return;
    const double* q = part + e * nseg * 4;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, sw = 0.0;
    for (int s = 0; s < nseg; ++s) s0 += q[s * 4], s1 += q[s * 4 + 1], s2 += q[s * 4 + 2], sw += q[s * 4 + 3];
    out[e * 3] = (float)(s0 / sw);
    out[e * 3 + 1] = (float)(s1 / sw);
    out[e * 3 + 2] = (float)(s2 / sw);
}

// one table entry per wave: entry e = i S + j has roughness (i + 1/2) / S and NoV (j + 1/2) / S; lane l takes the nodes
// q = a n + b = l, l + 64, ... in order, then the fixed butterfly
__global__ __launch_bounds__(kThreads) void k_brdf_lut(int S, int n, float* out) {
    const int e = (int)blockIdx.x * (kThreads / 64) + (int)(threadIdx.x >> 6);
    if (e >= S * S) return;  // whole waves leave together
    const int lane = threadIdx.x & 63;
    const double r = ((double)(e / S) + 0.5) / (double)S, mu = ((double)(e % S) + 0.5) / (double)S;
    const double alpha = r * r, k = alpha / 2.0, a2m1 = alpha * alpha - 1.0;
    const double vx = sqrt(1.0 - mu * mu);
    const double g1v = mu / ((1.0 - k) * mu + k);
    double A = 0.0, B = 0.0;
    for (int q = lane; q < n * n; q += 64) {
        const double u = ((double)(q / n) + 0.5) / (double)n;
        const double phi = (2.0 * M_PI) * (((double)(q % n) + 0.5) / (double)n);
        const double c2 = (1.0 - u) / (1.0 + a2m1 * u);
        const double NoH = sqrt(c2), sh = sqrt(1.0 - c2);
        const double VoH = vx * (sh * cos(phi)) + mu * NoH;
        const double NoL = (2.0 * VoH) * NoH - mu;
        if (NoL > 0.0 && VoH > 0.0) {
            const double g1l = NoL / ((1.0 - k) * NoL + k);
            const double Gv = ((g1l * g1v) * VoH) / (NoH * mu);
            const double Fc = exp2(-(5.55473 * VoH + 6.98316) * VoH);
            A += (1.0 - Fc) * Gv;
            B += Fc * Gv;
        }
    }
    A = wave_sum(A);
    B = wave_sum(B);
    if (lane == 0) {
        const double nn = (double)n * (double)n;
        out[(int64_t)e * 2] = (float)(A / nn);
        out[(int64_t)e * 2 + 1] = (float)(B / nn);
    }
}

// bilinear fetch of a cube strip [3, 6 S, S] at direction d: image_pos and bilinear_taps (pn_rays.h) in fp64, the taps
// clamped within the face; NaN for a zero or NaN direction
__device__ __forceinline__ void cube_fetch(const float* strip, int S, const double d[3], double out[3]) {
    double px, py;
    int face;
    if (!image_pos<double>(PN_CAM_CUBE, 6 * S, S, nullptr, d, px, py, face)) {
        out[0] = out[1] = out[2] = (double)NAN;
        return;
    }
    const Taps<double, int64_t> t = bilinear_taps<double, int64_t>(PN_CAM_CUBE, 6 * S, S, px, py, face);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* ch = strip + (int64_t)c * 6 * S * S;
        out[c] = ((t.w[0] * (double)ch[t.o[0]] + t.w[1] * (double)ch[t.o[1]]) + t.w[2] * (double)ch[t.o[2]]) +
                 t.w[3] * (double)ch[t.o[3]];
    }
}

struct IblMaps {
    const float* spec;  // levels l = 0 .. levels - 1 one after the other, each [3, 6 S_l, S_l], S_l = size >> l
    int size, levels;
    const float* irr;  // [3, 6 irr_size, irr_size]
    int irr_size;
    const float* lut;  // [lut_size, lut_size, 2]
    int lut_size;
};

// the engine's evaluation of row r: specular light = trilinear fetch along Rr at level roughness (levels - 1),
// E = the irradiance cube at n, (A, B) = the table at (NoV, roughness)
__global__ __launch_bounds__(kThreads) void k_ibl_shade(int64_t R, IblMaps m, const float* albedo, const float* normals,
                                                       const float* viewdirs, const float* roughness, float roughness_all,
                                                       float f0, float* rgb, float* diffuse, float* specular) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const double n[3] = {normals[r * 3], normals[r * 3 + 1], normals[r * 3 + 2]};
    const double dx = viewdirs[r * 3], dy = viewdirs[r * 3 + 1], dz = viewdirs[r * 3 + 2];
    const double dn = sqrt((dx * dx + dy * dy) + dz * dz);
    const double v[3] = {-(dx / dn), -(dy / dn), -(dz / dn)};
    const double nv = (n[0] * v[0] + n[1] * v[1]) + n[2] * v[2];
    const double NoV = nv < 0.0 ? 0.0 : nv;
    double refl[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) refl[k] = (2.0 * nv) * n[k] - v[k];
    const double rough = roughness ? (double)roughness[r] : (double)roughness_all;
    // specular light: the two levels around lambda
    int l0;
    double f;
    clamped_cell(rough * (double)(m.levels - 1), m.levels - 1, l0, f);
    const float* lv = m.spec;
    for (int l = 0; l < l0; ++l) lv += (int64_t)18 * (m.size >> l) * (m.size >> l);
    double a[3], b[3], E[3];
    cube_fetch(lv, m.size >> l0, refl, a);  // l0 <= levels - 2: at lambda = levels - 1 the upper level has weight 1
    cube_fetch(lv + (int64_t)18 * (m.size >> l0) * (m.size >> l0), m.size >> (l0 + 1), refl, b);
    cube_fetch(m.irr, m.irr_size, n, E);
    // (A, B), bilinear in the table
    int xi, yi;
    double tx, ty;
    const int S = m.lut_size;
    clamped_cell(NoV * (double)S - 0.5, S - 1, xi, tx);
    clamped_cell(rough * (double)S - 0.5, S - 1, yi, ty);
    const float* t00 = m.lut + ((int64_t)yi * S + xi) * 2;
    const float* t10 = t00 + (int64_t)S * 2;
    const double w00 = (1.0 - ty) * (1.0 - tx), w01 = (1.0 - ty) * tx, w10 = ty * (1.0 - tx), w11 = ty * tx;
    const double A = ((w00 * (double)t00[0] + w01 * (double)t00[2]) + w10 * (double)t10[0]) + w11 * (double)t10[2];
    const double B = ((w00 * (double)t00[1] + w01 * (double)t00[3]) + w10 * (double)t10[1]) + w11 * (double)t10[3];
    const double scale = (double)f0 * A + B;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double light = (1.0 - f) * a[c] + f * b[c];
        const double df = (double)albedo[r * 3 + c] / M_PI * E[c];
        const double sf = light * scale;
        diffuse[r * 3 + c] = (float)df;
        specular[r * 3 + c] = (float)sf;
        rgb[r * 3 + c] = (float)(df + sf);
    }
}

// the shape limits of pn_probe_irradiance, and K (P ceil(K / 256) segments workgroups < 2^31)
int check_prefilter(int64_t P, int H, int W, int64_t K) {
    if (P <= 0 || H < 2 || W < 2 || P >= (1 << 25) || (int64_t)H * W >= ((int64_t)1 << 30) || K <= 0 ||
        K >= ((int64_t)1 << 31))
        return PN_ERR_BAD_SHAPE;
    if (P * (int64_t)nblk(K, kThreads) * split_of((int64_t)H * W).segs >= ((int64_t)1 << 31)) return PN_ERR_BAD_SHAPE;
    return PN_OK;
}

}  // namespace

extern "C" {

int64_t pn_prefilter_work_doubles(int64_t P, int H, int W, int64_t K) {
    const int st = check_prefilter(P, H, W, K);
    if (st != PN_OK) return st;
    return P * K * split_of((int64_t)H * W).segs * 4;
}

int pn_prefilter(int64_t P, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps, const float* dirs,
                 const float* omega, int64_t K, const float* directions, int per_probe_directions, double roughness,
                 float* out, double* work, void* stream) {
    const int st = check_prefilter(P, H, W, K);
    if (st != PN_OK) return st;
    if (!(roughness > 0.0 && roughness <= 1.0)) return PN_ERR_BAD_SHAPE;
    if (!x || !dirs || !omega || !directions || !out || !work) return PN_ERR_NULL;
    const int64_t HW = (int64_t)H * W;
    const Split sp = split_of(HW);
    const int nkb = (int)nblk(K, kThreads);
    const double alpha = roughness * roughness;
    hipLaunchKernelGGL(k_prefilter, dim3((unsigned)(P * nkb * sp.segs)), dim3(kThreads), 0, ST(stream), HW, K, nkb, sp.segs,
                       sp.tiles, Probes{x, probe_stride, cs, ps}, dirs, omega, directions,
                       per_probe_directions ? K * 3 : (int64_t)0, alpha * alpha - 1.0, work);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_prefilter_finish, dim3(nblk(P * K, kThreads)), dim3(kThreads), 0, ST(stream), P * K, sp.segs, work,
                       out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_brdf_lut(int size, int samples, float* out, void* stream) {
    if (size < 2 || size > kMaxLut || samples < 1 || samples > kMaxLut) return PN_ERR_BAD_SHAPE;
    if (!out) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_brdf_lut, dim3(nblk((int64_t)size * size, kThreads / 64)), dim3(kThreads), 0, ST(stream), size,
                       samples, out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_ibl_shade(int64_t R, int size, int levels, const float* specular_levels, int irradiance_size,
                 const float* irradiance, int lut_size, const float* lut, const float* albedo, const float* normals,
                 const float* viewdirs, const float* roughness, float roughness_all, float f0, float* rgb, float* diffuse,
                 float* specular, void* stream) {
    if (R < 0 || R >= ((int64_t)1 << 31) * kThreads || size < 1 || size > kMaxLut || levels < 2 || levels > 13 || (size >> (levels - 1)) < 1 ||
        irradiance_size < 1 || irradiance_size > kMaxLut || lut_size < 2 || lut_size > kMaxLut)
        return PN_ERR_BAD_SHAPE;
    if (R == 0) return PN_OK;
    if (!specular_levels || !irradiance || !lut || !albedo || !normals || !viewdirs || !rgb || !diffuse || !specular)
        return PN_ERR_NULL;
    const IblMaps m{specular_levels, size, levels, irradiance, irradiance_size, lut, lut_size};
    hipLaunchKernelGGL(k_ibl_shade, dim3(nblk(R, kThreads)), dim3(kThreads), 0, ST(stream), R, m, albedo, normals, viewdirs,
                       roughness, roughness_all, f0, rgb, diffuse, specular);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
