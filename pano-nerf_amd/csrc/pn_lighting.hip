// pn_lighting.hip — spatially-varying lighting of a trained radiance field (gfx950): spherical-harmonic projection of
// HDR light probes, the exact cosine-weighted irradiance quadrature of a probe and trilinear sampling of an SH
// irradiance volume.  Conventions (pixel directions, solid angles, SH order and constants) are stated in
// include/panonerf_hip.h.
//
// Every sum runs in fp64 in a fixed order: the projection writes one row of partial sums per workgroup to the caller's
// workspace and a second launch adds the rows in order (the pn_metrics.hip pattern); the quadrature gives each thread
// one (probe, normal) pair and walks the pixels in order.  No atomics: two calls on the same inputs give the same bits.
// Radiance is read in place through (probe, channel, pixel) strides, so [P, 3, H, W] views of [P, H, W, 3] buffers
// need no copy.
#include "pn_common.h"
#include "pn_probes.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kShQ = 27;            // 9 coefficients x 3 channels
constexpr int kPixPerBlock = 2048;  // pixels one projection workgroup covers at least
constexpr int kMaxShBlocks = 64;    // projection workgroups per probe at most
constexpr int kTile = 256;          // pixels staged per LDS tile of the quadrature

// projection workgroups per probe: a function of the pixel count only, so a probe's sums do not depend on P
inline int sh_blocks(int64_t hw) {
    int64_t b = (hw + kPixPerBlock - 1) / kPixPerBlock;
    return (int)(b < kMaxShBlocks ? b : kMaxShBlocks);
}

// workgroup g = p * nb + b: partial SH sums of probe p over the pixels b, b + nb, ... (in blocks of kThreads):
// part[g * 27 + k * 3 + c] = sum L_c(pix) Y_k(dir_pix) omega_pix
__global__ __launch_bounds__(kThreads) void k_probe_sh(int64_t HW, int nb, Probes pr, const float* dirs,
                                                      const float* omega, double* part) {
    const int64_t p = blockIdx.x / nb;
    const int b = (int)(blockIdx.x % nb);
    const float* xp = pr.x + p * pr.probe_stride;
    double acc[kShQ];
#pragma unroll
    for (int q = 0; q < kShQ; ++q) acc[q] = 0.0;
    for (int64_t pix = (int64_t)b * kThreads + threadIdx.x; pix < HW; pix += (int64_t)nb * kThreads) {
        double Y[9];
        sh_basis<2>(dirs[pix * 3], dirs[pix * 3 + 1], dirs[pix * 3 + 2], Y);
        const double w = omega[pix];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double lw = (double)xp[c * pr.cs + pix * pr.ps] * w;
#pragma unroll
            for (int k = 0; k < 9; ++k) acc[k * 3 + c] += lw * Y[k];
        }
    }
    // fixed butterfly per wave, then the four waves in order
    __shared__ double red[kShQ][kThreads / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < kShQ; ++q) {
        const double s = wave_sum(acc[q]);
        if (lane == 0) red[q][wv] = s;
    }
    __syncthreads();
    if (threadIdx.x < kShQ) {
        double s = red[threadIdx.x][0];
        for (int w = 1; w < kThreads / 64; ++w) s += red[threadIdx.x][w];
        part[(int64_t)blockIdx.x * kShQ + threadIdx.x] = s;
    }
}

// out[p, k, c] = sum over the nb partial rows of probe p, in order
__global__ __launch_bounds__(kThreads) void k_probe_sh_finish(int64_t P, int nb, const double* part, float* out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= P * kShQ) return;
    const int64_t p = e / kShQ;
    const int q = (int)(e % kShQ);
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[(p * nb + b) * kShQ + q];
    out[e] = (float)s;
}

// E[p, n] = sum_pix L_p(pix) max(0, n . dir_pix) omega_pix: workgroup g = p * nkb + b takes normals b * 256 .. b * 256
// + 255 of probe p, one per thread; the probe's (L omega, dir) go through LDS in tiles of kTile pixels, as fp64 (the
// product of two fp32 values is exact there).  relu as torch evaluates it: a NaN dot product stays NaN.
__global__ __launch_bounds__(kThreads) void k_probe_irradiance(int64_t HW, int64_t K, int nkb, Probes pr, const float* dirs,
                                                              const float* omega, const float* normals,
                                                              int64_t normal_stride, float* out) {
    __shared__ double4 s_dir[kTile], s_rad[kTile];
    const int64_t p = blockIdx.x / nkb;
    const int64_t n = (int64_t)(blockIdx.x % nkb) * kThreads + threadIdx.x;
    const float* xp = pr.x + p * pr.probe_stride;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (n < K) {
        const float* np_ = normals + p * normal_stride + n * 3;
        nx = np_[0], ny = np_[1], nz = np_[2];
    }
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    for (int64_t base = 0; base < HW; base += kTile) {
        const int cnt = (int)((HW - base) < kTile ? (HW - base) : kTile);
        for (int t = threadIdx.x; t < cnt; t += kThreads) {
            const int64_t pix = base + t;
            const double w = omega[pix];
            s_dir[t] = make_double4(dirs[pix * 3], dirs[pix * 3 + 1], dirs[pix * 3 + 2], 0.0);
            s_rad[t] = make_double4((double)xp[pix * pr.ps] * w, (double)xp[pr.cs + pix * pr.ps] * w,
                                    (double)xp[2 * pr.cs + pix * pr.ps] * w, 0.0);
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const double4 d = s_dir[t];
            double c = nx * d.x + ny * d.y + nz * d.z;
            c = c < 0.0 ? 0.0 : c;
            const double4 r = s_rad[t];
            e0 += r.x * c;
            e1 += r.y * c;
            e2 += r.z * c;
        }
        __syncthreads();
    }
    if (n < K) {
        float* o = out + (p * K + n) * 3;
        o[0] = (float)e0;
        o[1] = (float)e1;
        o[2] = (float)e2;
    }
}

struct Volume {
    int n[3];
    float o[3], d[3];  // vertex (i, j, k) at o + (i, j, k) * d, as pn_grid_points places it
};

// continuous grid coordinate of x on axis a, clamped to [0, n - 1] (NaN passes through): cell index and weight
__device__ __forceinline__ void axis_cell(const Volume& v, int a, double x, int& i, double& t) {
    double u = v.d[a] != 0.f ? (x - (double)v.o[a]) / (double)v.d[a] : 0.0;
    clamped_cell(u, v.n[a] - 1, i, t);  // top >= 1: pn_sh_volume_irradiance refuses an axis of fewer than 2 vertices
}

// E(n) = sum_lm A_l L_lm Y_lm(n), L_lm interpolated trilinearly from the 8 vertices around the clamped point
__global__ __launch_bounds__(kThreads) void k_sh_volume_irradiance(int64_t M, Volume v, const float* sh,
                                                                  const float* points, const float* normals,
                                                                  float* out) {
    const int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (m >= M) return;
    int ci[3];
    double t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) axis_cell(v, a, (double)points[m * 3 + a], ci[a], t[a]);
    double L[kShQ];
#pragma unroll
    for (int q = 0; q < kShQ; ++q) L[q] = 0.0;
    for (int corner = 0; corner < 8; ++corner) {
        const int bi = corner >> 2, bj = (corner >> 1) & 1, bk = corner & 1;
        const double w = (bi ? t[0] : 1.0 - t[0]) * (bj ? t[1] : 1.0 - t[1]) * (bk ? t[2] : 1.0 - t[2]);
        const int64_t vid = ((int64_t)(ci[0] + bi) * v.n[1] + (ci[1] + bj)) * v.n[2] + (ci[2] + bk);
        const float* s = sh + vid * kShQ;
#pragma unroll
        for (int q = 0; q < kShQ; ++q) L[q] += w * (double)s[q];
    }
    double Y[9];
    sh_basis<2>(normals[m * 3], normals[m * 3 + 1], normals[m * 3 + 2], Y);
    const double A[9] = {M_PI, 2.0 * M_PI / 3.0, 2.0 * M_PI / 3.0, 2.0 * M_PI / 3.0, M_PI / 4.0, M_PI / 4.0,
                         M_PI / 4.0, M_PI / 4.0, M_PI / 4.0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double e = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) e += (A[k] * Y[k]) * L[k * 3 + c];
        out[m * 3 + c] = (float)e;
    }
}

// P < 2^25 probes (P * 64 projection workgroups < 2^31) of H x W < 2^30 pixels, H and W >= 2
int check_probes(int64_t P, int H, int W, const float* x, const float* dirs, const float* omega) {
    if (P <= 0 || H < 2 || W < 2 || P >= (1 << 25) || (int64_t)H * W >= ((int64_t)1 << 30)) return PN_ERR_BAD_SHAPE;
    if (!x || !dirs || !omega) return PN_ERR_NULL;
    return PN_OK;
}

}  // namespace

extern "C" {

int64_t pn_probe_sh_work_doubles(int64_t P, int H, int W) {
    if (P <= 0 || H < 2 || W < 2 || P >= (1 << 25) || (int64_t)H * W >= ((int64_t)1 << 30)) return PN_ERR_BAD_SHAPE;
    return P * sh_blocks((int64_t)H * W) * kShQ;
}

int pn_probe_sh(int64_t P, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps,
                const float* dirs, const float* omega, float* out, double* work, void* stream) {
    int st = check_probes(P, H, W, x, dirs, omega);
    if (st != PN_OK) return st;
    if (!out || !work) return PN_ERR_NULL;
    const int64_t HW = (int64_t)H * W;
    const int nb = sh_blocks(HW);
    hipLaunchKernelGGL(k_probe_sh, dim3((unsigned)(P * nb)), dim3(kThreads), 0, ST(stream), HW, nb,
                       Probes{x, probe_stride, cs, ps}, dirs, omega, work);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_probe_sh_finish, dim3(nblk(P * kShQ, kThreads)), dim3(kThreads), 0, ST(stream), P, nb, work,
                       out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_probe_irradiance(int64_t P, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps,
                        const float* dirs, const float* omega, int64_t K, const float* normals, int per_probe_normals,
                        float* out, void* stream) {
    int st = check_probes(P, H, W, x, dirs, omega);
    if (st != PN_OK) return st;
    if (K <= 0 || P * (int64_t)nblk(K, kThreads) >= ((int64_t)1 << 31)) return PN_ERR_BAD_SHAPE;
    if (!normals || !out) return PN_ERR_NULL;
    const int nkb = (int)nblk(K, kThreads);
    hipLaunchKernelGGL(k_probe_irradiance, dim3((unsigned)(P * nkb)), dim3(kThreads), 0, ST(stream), (int64_t)H * W, K, nkb,
                       Probes{x, probe_stride, cs, ps}, dirs, omega, normals, per_probe_normals ? K * 3 : (int64_t)0,
                       out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_sh_volume_irradiance(int nx, int ny, int nz, float x0, float y0, float z0, float dx, float dy, float dz,
                            const float* sh, int64_t M, const float* points, const float* normals, float* out,
                            void* stream) {
    if (nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny * nz >= ((int64_t)1 << 31) || M < 0) return PN_ERR_BAD_SHAPE;
    if (M == 0) return PN_OK;
    if (!sh || !points || !normals || !out) return PN_ERR_NULL;
    Volume v{{nx, ny, nz}, {x0, y0, z0}, {dx, dy, dz}};
    hipLaunchKernelGGL(k_sh_volume_irradiance, dim3(nblk(M, kThreads)), dim3(kThreads), 0, ST(stream), M, v, sh,
                       points, normals, out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
