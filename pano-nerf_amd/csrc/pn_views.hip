// pn_views.hip — novel views (gfx950): the viewable uint8 frames the reference's validation writes (tone-mapped LDR,
// hotmap depth, (n + 1) / 2 normals, albedo).  The rays of a view come from pn_cameras.hip.  Conventions are stated in
// include/panonerf_hip.h.
//
// Frames: one thread per pixel; the depth kind first reduces (min, max) of the normalised depth over the image in one
// workgroup, in a fixed order and without atomics, so that repeated calls give the same bytes.  Images are read in place
// through (channel, pixel) strides, as pn_metrics.hip reads them.
#include "pn_common.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMinMaxThreads = 1024;

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
