// pn_views.hip — novel views (gfx950): pinhole (perspective) ray generation from (camera, pixel) and the viewable
// uint8 frames the reference's validation writes (tone-mapped LDR, hotmap depth, (n + 1) / 2 normals, albedo).
// Conventions are stated in include/panonerf_hip.h.
//
// Rays: one thread per batch ray regenerates it from the camera's pix2cam and c2w, the mip-NeRF cone radius included
// (the neighbour's direction is recomputed in the thread, so no ray pool is stored).  Frames: one thread per pixel;
// the depth kind first reduces (min, max) of the normalised depth over the image in one workgroup, in a fixed order and
// without atomics, so that repeated calls give the same bytes.  Images are read in place through (channel, pixel) strides,
// as pn_metrics.hip reads them.
#include "pn_common.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMinMaxThreads = 1024;

#define ST(s) ((hipStream_t)(s))

__host__ __device__ inline unsigned nblk(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }

// c2w[:3,:3] @ (pix2cam @ (px, py, 1)), each a 3-term fp32 dot product in index order
__device__ __forceinline__ void pinhole_dir(const float* p2c, const float* c2w, float px, float py, float out[3]) {
    float cam[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) cam[k] = (p2c[3 * k] * px + p2c[3 * k + 1] * py) + p2c[3 * k + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (c2w[4 * k] * cam[0] + c2w[4 * k + 1] * cam[1]) + c2w[4 * k + 2] * cam[2];
}

// batch ray b is pixel idx[b] % (H W) of camera idx[b] / (H W) (an index outside the pool reads ray 0, as
// k_sample_pano_rays does).  radius = |d(i, j) - d(i + 1, j)| * 2 / sqrt(12); the last row reuses row H - 2's value
__global__ __launch_bounds__(kThreads) void k_sample_pinhole_rays(int64_t B, int n_cam, int H, int W, const int64_t* idx,
                                                                  const float* pix2cams, const float* c2ws, float near_,
                                                                  float far_, const float* rgb_pool, float* origins,
                                                                  float* directions, float* viewdirs, float* radii,
                                                                  float* lossmult, float* near_out, float* far_out,
                                                                  float* noise_var, float* rgb_out) {
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    const int64_t hw = (int64_t)H * W;
    int64_t r = idx[b];
    r = (r >= 0 && r < hw * n_cam) ? r : 0;
    const int cam = (int)(r / hw);
    const int pix = (int)(r % hw);
    const int i = pix / W, j = pix % W;
    const float* p2c = pix2cams + 9 * (int64_t)cam;
    const float* m = c2ws + 16 * (int64_t)cam;
    const float px = (float)j + 0.5f;
    float d[3], a[3], n[3];
    pinhole_dir(p2c, m, px, (float)i + 0.5f, d);
    const int ii = i < H - 1 ? i : H - 2;
    pinhole_dir(p2c, m, px, (float)ii + 0.5f, a);
    pinhole_dir(p2c, m, px, (float)(ii + 1) + 0.5f, n);
    const float dx = sqrtf((a[0] - n[0]) * (a[0] - n[0]) + (a[1] - n[1]) * (a[1] - n[1]) + (a[2] - n[2]) * (a[2] - n[2]));
    const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    origins[b * 3 + 0] = m[3];
    origins[b * 3 + 1] = m[7];
    origins[b * 3 + 2] = m[11];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        directions[b * 3 + k] = d[k];
        viewdirs[b * 3 + k] = d[k] / nrm;
    }
    radii[b] = (float)((double)dx * 2.0 / sqrt(12.0));
    lossmult[b] = 1.f;
    near_out[b] = near_;
    far_out[b] = far_;
    noise_var[b] = 0.f;
    if (rgb_pool) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb_out[b * 3 + k] = rgb_pool[r * 3 + k];
    }
}

struct Src {
    const float* p;
    int64_t cs, ps;  // element (c, pix) at p[c * cs + pix * ps]
};

// the depth hotmap's input: (d - near) / (far - near), fp32 as torch evaluates it
__device__ __forceinline__ float depth_norm(const Src& s, int64_t pix, float near_, float range) {
    return (s.p[pix * s.ps] - near_) / range;
}

// numpy's min / max: a NaN anywhere makes the result NaN
__device__ __forceinline__ float nan_min(float a, float b) { return (isnan(a) || a < b) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (isnan(a) || a > b) ? a : b; }

// mm[0..1] = (min, max) of the normalised depth over the image: strided per thread, then a fixed tree
__global__ __launch_bounds__(kMinMaxThreads) void k_depth_minmax(int64_t HW, Src s, float near_, float range, float* mm) {
    __shared__ float smin[kMinMaxThreads], smax[kMinMaxThreads];
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t p = threadIdx.x; p < HW; p += kMinMaxThreads) {
        const float v = depth_norm(s, p, near_, range);
        lo = nan_min(lo, v);
        hi = nan_max(hi, v);
    }
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int o = kMinMaxThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            smin[threadIdx.x] = nan_min(smin[threadIdx.x], smin[threadIdx.x + o]);
            smax[threadIdx.x] = nan_max(smax[threadIdx.x], smax[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mm[0] = smin[0];
        mm[1] = smax[0];
    }
}

// (v * 255).astype(np.uint8) for v in [0, 1]; NaN gives 0
__device__ __forceinline__ uint8_t to_byte(float v) {
    const float t = truncf(v * 255.f);
    if (!(t >= 0.f)) return 0;
    return t >= 255.f ? (uint8_t)255 : (uint8_t)t;
}

// ||v|| as ATen's linalg_vector_norm evaluates three fp32 components (as pn_metrics.hip's k_normals)
__device__ __forceinline__ float norm3(float a, float b, float c) { return sqrtf(fmaf(c, c, fmaf(b, b, a * a))); }

__global__ __launch_bounds__(kThreads) void k_frame(int kind, int64_t HW, Src s, float scale, float near_, float range,
                                                    const float* mm, const float* lut, uint8_t* out) {
    const int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (pix >= HW) return;
    uint8_t* o = out + pix * 3;
    if (kind == PN_FRAME_DEPTH) {
        // hotmap: x - x.min() / (x.max() - x.min()) (the reference's precedence), then jet
        const float q = mm[0] / (mm[1] - mm[0]);
        float x = depth_norm(s, pix, near_, range) - q;
        const float* c;
        if (isnan(x)) {
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = 0;
            return;
        }
        x = x * 256.f;
        if (x == 256.f) x = 255.f;
        if (x < 0.f) c = lut;
        else if (x >= 256.f) c = lut + 255 * 3;
        else c = lut + 3 * (int)x;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = to_byte(c[k]);
        return;
    }
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = s.p[k * s.cs + pix * s.ps];
    if (kind == PN_FRAME_NORMAL) {
        // F.normalize(n, dim=channel), then (n + 1) / 2
        float n = norm3(v[0], v[1], v[2]);
        n = n < 1e-12f ? 1e-12f : n;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = to_byte((v[k] / n + 1.f) / 2.f);
    } else if (kind == PN_FRAME_ALBEDO) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = to_byte(clamp01(v[k]));
    } else {  // LDR (uint8 quantisation inside hdr_to_ldr) or LDR_GT (none)
        const int mode = kind == PN_FRAME_LDR ? 2 : 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = to_byte(tonemap(v[k] * scale, mode));
    }
}

}  // namespace

extern "C" {

int pn_sample_pinhole_rays(int64_t B, int n_cam, int H, int W, const int64_t* idx, const float* pix2cams,
                           const float* c2ws, float near_, float far_, const float* rgb_pool, float* origins,
                           float* directions, float* viewdirs, float* radii, float* lossmult, float* near_out,
                           float* far_out, float* noise_var, float* rgb_out, void* stream) {
    if (B <= 0 || n_cam <= 0 || H < 2 || W < 2 || (int64_t)H * W >= ((int64_t)1 << 31)) return PN_ERR_BAD_SHAPE;
    if (!idx || !pix2cams || !c2ws || !origins || !directions || !viewdirs || !radii || !lossmult || !near_out ||
        !far_out || !noise_var)
        return PN_ERR_NULL;
    if ((rgb_pool == nullptr) != (rgb_out == nullptr)) return PN_ERR_NULL;  // target colours: both or neither
    hipLaunchKernelGGL(k_sample_pinhole_rays, dim3(nblk(B, kThreads)), dim3(kThreads), 0, ST(stream), B, n_cam, H, W, idx,
                       pix2cams, c2ws, near_, far_, rgb_pool, origins, directions, viewdirs, radii, lossmult, near_out,
                       far_out, noise_var, rgb_out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_to_frame(int kind, int H, int W, const float* x, int64_t cs, int64_t ps, float scale, float near_, float range,
                const float* lut, float* work, uint8_t* out, void* stream) {
    if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) return PN_ERR_BAD_SHAPE;
    if (kind < PN_FRAME_LDR || kind > PN_FRAME_ALBEDO) return PN_ERR_UNSUPPORTED;
    if (!x || !out) return PN_ERR_NULL;
    if (kind == PN_FRAME_DEPTH && (!lut || !work)) return PN_ERR_NULL;
    const int64_t HW = (int64_t)H * W;
    const Src s{x, cs, ps};
    if (kind == PN_FRAME_DEPTH) {
        hipLaunchKernelGGL(k_depth_minmax, dim3(1), dim3(kMinMaxThreads), 0, ST(stream), HW, s, near_, range, work);
        PN_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_frame, dim3(nblk(HW, kThreads)), dim3(kThreads), 0, ST(stream), kind, HW, s, scale, near_, range,
                       work, lut, out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
