// pn_cameras.hip — cameras (gfx950): ray generation from (camera, pixel) for every camera model (panorama, pinhole,
// cube map, equidistant fisheye, stereo panorama (ODS)), the panorama pool generator, and reprojection and depth-aware
// warping of images between the central cameras (panorama, pinhole, cube map, fisheye).  Conventions are stated in include/panonerf_hip.h.
//
// Rays: one thread per batch ray regenerates it from the camera matrices, the cone radius included (the neighbour's
// direction is recomputed in the thread), so no 56-byte-per-ray pool is stored or read; only the 12-byte
// target colour is gathered.  One kernel template, k_sample_rays, instantiated per camera kind of pn_rays.h.
// Reprojection: one thread per (image, destination pixel), a gather: every subsample goes destination pixel ->
// direction -> rotated -> source pixel once, its four bilinear taps are reused over the channels (four accumulators at a
// time), the mean over the valid subsamples is taken in a fixed order, and consecutive lanes store consecutive pixels of
// a destination row.  No atomics.
// Warping: z-buffered forward splatting of RGB-D frames into other posed cameras (k_warp_splat, k_warp_resolve), further
// down beside the reprojection whose projections it shares.
#include "pn_rays.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kChan = 4;  // channels accumulated per pass over the subsamples

struct CamParams {
    float v[PN_CAM_PARAMS];
};
struct Rot {
    float m[9];
};

constexpr float kPi = PiOf<float>::value;

// ---------------------------------------------------------------------------------------------------- ray generation
// the pool of one panorama camera, row-major pixels
__global__ __launch_bounds__(kThreads) void k_raygen_pano(int H, int W, PanoCam c, float near_, float far_, RayOut out) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= H * W) return;
    store_ray(idx, pano_ray(H, W, c, idx / W, idx % W), near_, far_, out);
}

// batch ray b is pixel idx[b] % (H W) of camera idx[b] / (H W), with the target colour of that pool row
template <class Cam, int kBlock>
__global__ __launch_bounds__(kBlock) void k_sample_rays(int64_t B, int n_cam, Cam cam, const int64_t* idx, float near_,
                                                        float far_, const float* rgb_pool, RayOut out) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    const RowId r = decode_row(idx[b], (int64_t)cam.H * cam.W, n_cam);
    store_ray(b, cam.ray(r.cam, r.pix / cam.W, r.pix % cam.W), near_, far_, out);
    if (rgb_pool) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out.rgb_out[b * 3 + k] = rgb_pool[r.row * 3 + k];
    }
}

// the pointer checks every ray entry point makes: the eight fields are mandatory, target colours come both or neither
bool ray_ptrs_ok(const int64_t* idx, const float* c2ws, const float* rgb_pool, const RayOut& o) {
    if (!idx || !c2ws || !o.origins || !o.directions || !o.viewdirs || !o.radii || !o.lossmult || !o.near_out || !o.far_out ||
        !o.noise_var)
        return false;
    return (rgb_pool == nullptr) == (o.rgb_out == nullptr);
}

template <int kBlock, class Cam>
int launch_sample_rays(int64_t B, int n_cam, const Cam& cam, const int64_t* idx, float near_, float far_,
                       const float* rgb_pool, const RayOut& out, void* stream) {
    hipLaunchKernelGGL((k_sample_rays<Cam, kBlock>), dim3(nblk(B, kBlock)), dim3(kBlock), 0, ST(stream), B, n_cam, cam, idx,
                       near_, far_, rgb_pool, out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

// ------------------------------------------------------------------------------------------------------ reprojection
// destination position (px, py) -> camera-space direction (not normalised); false outside the camera's coverage
__device__ __forceinline__ bool dst_dir(int kind, int H, int W, const CamParams& p, float px, float py, float d[3]) {
    if (kind == PN_CAM_PANO) {
        const float theta = -(px / (float)W) * (2.f * kPi), phi = (py / (float)H) * kPi;
        float st, ct, sp, cp;
        sincosf(theta, &st, &ct);
        sincosf(phi, &sp, &cp);
        d[0] = sp * st, d[1] = cp, d[2] = sp * ct;
        return true;
    }
    if (kind == PN_CAM_PINHOLE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = (p.v[3 * k] * px + p.v[3 * k + 1] * py) + p.v[3 * k + 2];
        return true;
    }
    if (kind == PN_CAM_CUBE) {
        cube_dir(W, px, py, d);
        return true;
    }
    return fisheye_dir(H, W, p.v[0], px, py, d) <= p.v[1];
}

__global__ __launch_bounds__(kThreads) void k_reproject(int N, int C, int sk, int Hs, int Ws, CamParams sp, int dk, int Hd,
                                                        int Wd, CamParams dp, Rot rot, int samples, float fill,
                                                        const float* image, int64_t ns, int64_t cs, int64_t ps, float* out,
                                                        float* coverage) {
    const int64_t hw = (int64_t)Hd * Wd;
    const int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (pix >= hw) return;
    const int y = (int)(pix / Wd), x = (int)(pix % Wd);
    const float inv_k = 1.f / (float)samples;
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const float* img = image + (int64_t)n * ns;
        float* o = out + (int64_t)n * C * hw + pix;
        for (int c0 = 0; c0 < C; c0 += kChan) {
            float acc[kChan];
#pragma unroll
            for (int c = 0; c < kChan; ++c) acc[c] = 0.f;
            int valid = 0;
            for (int b = 0; b < samples; ++b) {
                for (int a = 0; a < samples; ++a) {
                    const float px = (float)x + ((float)a + 0.5f) * inv_k, py = (float)y + ((float)b + 0.5f) * inv_k;
                    float d[3], e[3], qx, qy;
                    int face;
                    if (!dst_dir(dk, Hd, Wd, dp, px, py, d)) continue;
                    rotate3(rot.m, 3, d, e);
                    if (!image_pos(sk, Hs, Ws, sp.v, e, qx, qy, face)) continue;
                    const Taps<float, int> t = bilinear_taps<float, int>(sk, Hs, Ws, qx, qy, face);
                    ++valid;
#pragma unroll
                    for (int c = 0; c < kChan; ++c) {
                        if (c0 + c < C) {
                            const float* ch = img + (int64_t)(c0 + c) * cs;
                            const float v = ((t.w[0] * ch[t.o[0] * ps] + t.w[1] * ch[t.o[1] * ps]) + t.w[2] * ch[t.o[2] * ps]) +
                                            t.w[3] * ch[t.o[3] * ps];
                            acc[c] = acc[c] + v;
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < kChan; ++c) {
                if (c0 + c < C) o[(int64_t)(c0 + c) * hw] = valid ? acc[c] / (float)valid : fill;
            }
            if (n == 0 && c0 == 0) coverage[pix] = (float)valid / (float)(samples * samples);
        }
    }
}

// ------------------------------------------------------------------------------------------------ depth-aware warping
// z-buffered forward splatting of RGB-D frames (pn_warp_splat, pn_warp_resolve; formulas in include/panonerf_hip.h).
// Splat: one thread per (source frame, source pixel) lifts its pixel to a world point once, then for every destination
// (gridDim.y, as k_reproject's images) projects it and takes a 64-bit minimum of (rho bits, source index) over its
// footprint: plain no-return global 64-bit vector atomics, keys unique, so the result is independent of their order.
// Resolve: one thread per (destination, pixel) decodes the key and gathers.  No LDS, no scratch.

// unit camera-space direction of the centre of pixel (i, j) (a fisheye's equidistant formula outside its circle too)
__device__ __forceinline__ void unit_dir(int kind, int H, int W, const CamParams& p, int i, int j, float d[3]) {
    dst_dir(kind, H, W, p, (float)j + 0.5f, (float)i + 0.5f, d);
    if (kind == PN_CAM_PINHOLE || kind == PN_CAM_CUBE) normalize3(d);
}

// |u(y, j) - u(y + 1, j)| of the unit directions, rows as row_step_radius counts them: within a cube's face, the last
// row reusing the one before
__device__ __forceinline__ float row_step(int kind, int H, int W, const CamParams& p, int i, int j) {
    const int rows = kind == PN_CAM_CUBE ? W : H;
    const int top = kind == PN_CAM_CUBE ? (i / W) * W : 0;
    const int y = i - top;
    const int yy = y < rows - 1 ? y : rows - 2;
    float a[3], n[3];
    unit_dir(kind, H, W, p, top + yy, j, a);
    unit_dir(kind, H, W, p, top + yy + 1, j, n);
    return sqrtf(((a[0] - n[0]) * (a[0] - n[0]) + (a[1] - n[1]) * (a[1] - n[1])) + (a[2] - n[2]) * (a[2] - n[2]));
}

__device__ __forceinline__ float norm3(const float d[3]) { return sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]); }

__global__ __launch_bounds__(kThreads) void k_warp_splat(int64_t n_src, int sk, int Hs, int Ws, CamParams sp,
                                                         const float* depth, const float* src_c2ws, int D, int dk, int Hd,
                                                         int Wd, CamParams dp, const float* dst_c2ws, int max_splat,
                                                         float scale, unsigned long long* zbuf) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n_src) return;
    const float t = depth[idx];
    if (!(t > 0.f && t < INFINITY)) return;
    const int64_t hws = (int64_t)Hs * Ws;
    const int pix = (int)(idx % hws);
    const int i = pix / Ws, j = pix % Ws;
    const float* m = src_c2ws + 16 * (idx / hws);
    // the world direction of the pixel's ray, with the arithmetic of the ray kernels (pn_rays.h), and |dc|
    float w[3], nd = 1.f;
    if (sk == PN_CAM_PANO) {
        const float theta = -((float)j + 0.5f) / (float)Ws * 2.f * kPi;
        const float phi = ((float)i + 0.5f) / (float)Hs * kPi;
        const float s_ = sinf(phi);
        const float x = s_ * sinf(theta), y = cosf(phi), z = s_ * cosf(theta);
        w[0] = x * m[0] + y * m[1] + z * m[2];
        w[1] = x * m[4] + y * m[5] + z * m[6];
        w[2] = x * m[8] + y * m[9] + z * m[10];
    } else {
        float c[3];
        if (!dst_dir(sk, Hs, Ws, sp, (float)j + 0.5f, (float)i + 0.5f, c)) return;  // outside a fisheye's circle
        if (sk == PN_CAM_CUBE) normalize3(c);
        if (sk == PN_CAM_PINHOLE) nd = norm3(c);
        rotate3(m, 4, c, w);
    }
    float X[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = w[k] * t + m[4 * k + 3];
    const float num = scale * ((t * nd) * row_step(sk, Hs, Ws, sp, i, j));
    const int64_t hwd = (int64_t)Hd * Wd;
    const int rows = dk == PN_CAM_CUBE ? Wd : Hd;
    for (int d = blockIdx.y; d < D; d += gridDim.y) {
        const float* md = dst_c2ws + 16 * (int64_t)d;
        float v[3], e[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = X[k] - md[4 * k + 3];
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = (md[k] * v[0] + md[4 + k] * v[1]) + md[8 + k] * v[2];  // R_d^T v
        const float rho = norm3(e);
        if (!(rho > 0.f && rho < INFINITY)) continue;
        float qx, qy;
        int face;
        if (!image_pos(dk, Hd, Wd, dp.v, e, qx, qy, face)) continue;
        const int top = dk == PN_CAM_CUBE ? face * Wd : 0;
        // the landing pixel, kept inside the image (a position on the last border lands in the last pixel)
        int lx = (int)floorf(qx), ly = (int)floorf(qy);
        lx = lx < 0 ? 0 : (lx > Wd - 1 ? Wd - 1 : lx);
        ly = ly < 0 ? 0 : (ly > rows - 1 ? rows - 1 : ly);
        const float size = num / (rho * row_step(dk, Hd, Wd, dp, top + ly, lx));
        int k = 1;
        if (size > 1.f) k = size >= (float)max_splat ? max_splat : (int)ceilf(size);
        const float half = (float)(k - 1) * 0.5f;
        const int x0 = (int)floorf(qx - half), y0 = (int)floorf(qy - half);
        const unsigned long long key = ((unsigned long long)__float_as_uint(rho) << 32) | (unsigned long long)(uint32_t)idx;
        unsigned long long* zb = zbuf + (int64_t)d * hwd;
        for (int b = 0; b < k; ++b) {
            const int y = y0 + b;
            if (y < 0 || y >= rows) continue;
            for (int a = 0; a < k; ++a) {
                int x = x0 + a;
                if (dk == PN_CAM_PANO) x = ((x % Wd) + Wd) % Wd;
                else if (x < 0 || x >= Wd) continue;
                atomicMin(zb + (int64_t)(top + y) * Wd + x, key);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_warp_resolve(int64_t n_src, int C, int Hs, int Ws, int64_t n_dst, int dk, int Hd,
                                                           int Wd, CamParams dp, const unsigned long long* zbuf,
                                                           const float* image, int64_t ns, int64_t cs, int64_t ps, float fill,
                                                           float* out, float* depth_out, int64_t* index, float* coverage) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n_dst) return;
    const int64_t hwd = (int64_t)Hd * Wd, hws = (int64_t)Hs * Ws;
    const int64_t d = idx / hwd, pix = idx % hwd;
    const unsigned long long key = zbuf[idx];
    const int64_t src = (int64_t)(key & 0xffffffffull);
    const bool hit = key != PN_WARP_EMPTY && src < n_src;  // a key no splat of these sources wrote reads as empty
    float dep = NAN;
    if (hit) {
        dep = __uint_as_float((unsigned)(key >> 32));
        if (dk == PN_CAM_PINHOLE) {
            float c[3];
            dst_dir(dk, Hd, Wd, dp, (float)(pix % Wd) + 0.5f, (float)(pix / Wd) + 0.5f, c);
            dep = dep / norm3(c);
        }
    }
    depth_out[idx] = dep;
    index[idx] = hit ? src : -1;
    coverage[idx] = hit ? 1.f : 0.f;
    if (!out) return;
    const float* px = hit ? image + (src / hws) * ns + (src % hws) * ps : nullptr;
    float* o = out + d * C * hwd + pix;
    for (int c = 0; c < C; ++c) o[(int64_t)c * hwd] = hit ? px[(int64_t)c * cs] : fill;
}

// blend S layers of warped frames per destination pixel: the layers on the nearest surface, by weight (pn_warp_blend)
__global__ __launch_bounds__(kThreads) void k_warp_blend(int S, int64_t D, int C, int64_t hw, const float* images,
                                                         const float* depths, const float* weights, float q, float fill,
                                                         float* out, float* depth_out, float* coverage) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= D * hw) return;
    const int64_t d = idx / hw, pix = idx % hw;
    const int64_t zs = D * hw, vs = D * C * hw;  // layer strides of depths and images
    const float* z = depths + idx;
    float zn = INFINITY;
    for (int s = 0; s < S; ++s) {
        const float t = z[s * zs];
        if (t > 0.f && t < zn) zn = t;  // NaN, 0, negative and Inf are no points
    }
    float* o = out + d * C * hw + pix;
    if (!(zn < INFINITY)) {
        depth_out[idx] = NAN;
        coverage[idx] = 0.f;
        for (int c = 0; c < C; ++c) o[(int64_t)c * hw] = fill;
        return;
    }
    int kept = 0, one = 0;
    float wsum = 0.f;
    for (int s = 0; s < S; ++s) {
        const float t = z[s * zs];
        if (!(t > 0.f && t < INFINITY && t * q <= zn)) continue;
        const float w = weights[s * D + d];
        wsum = kept ? wsum + w : w;
        one = kept ? one : s;
        ++kept;
    }
    coverage[idx] = 1.f;
    const float* v = images + d * C * hw + pix;
    if (kept == 1) {  // a single source keeps its bits
        depth_out[idx] = z[one * zs];
        for (int c = 0; c < C; ++c) o[(int64_t)c * hw] = v[one * vs + (int64_t)c * hw];
        return;
    }
    for (int c = 0; c <= C; ++c) {
        float acc = 0.f;
        bool first = true;
        for (int s = 0; s < S; ++s) {
            const float t = z[s * zs];
            if (!(t > 0.f && t < INFINITY && t * q <= zn)) continue;
            const float x = weights[s * D + d] * (c == C ? t : v[s * vs + (int64_t)c * hw]);
            acc = first ? x : acc + x;
            first = false;
        }
        if (c == C) depth_out[idx] = acc / wsum;
        else o[(int64_t)c * hw] = acc / wsum;
    }
}

// minimum image size of a camera kind; false for an unknown kind
bool min_size(int kind, int H, int W, bool& ok) {
    switch (kind) {
        case PN_CAM_PANO: ok = H >= 2 && W >= 3; return true;
        case PN_CAM_STEREO_PANO: ok = H >= 2 && W >= 3; return true;
        case PN_CAM_PINHOLE: ok = H >= 2 && W >= 2; return true;
        case PN_CAM_FISHEYE: ok = H >= 2 && W >= 2; return true;
        case PN_CAM_CUBE: ok = W >= 2 && (int64_t)H == 6 * (int64_t)W; return true;
        default: return false;
    }
}

}  // namespace

extern "C" {

int pn_raygen_pano(int H, int W, const float* c, float near_, float far_, float* origins, float* directions,
                   float* viewdirs, float* radii, float* lossmult, float* near_out, float* far_out, float* noise_var,
                   void* stream) {
    if (H <= 0 || W < 3) return PN_ERR_BAD_SHAPE;
    if (!c || !origins || !directions || !viewdirs || !radii || !lossmult || !near_out || !far_out || !noise_var)
        return PN_ERR_NULL;
    const RayOut out{origins, directions, viewdirs, radii, lossmult, near_out, far_out, noise_var, nullptr};
    hipLaunchKernelGGL(k_raygen_pano, dim3(nblk((int64_t)H * W, kThreads)), dim3(kThreads), 0, ST(stream), H, W, pano_cam(c), near_,
                       far_, out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_sample_pano_rays(int64_t B, int n_cam, int H, int W, const int64_t* idx, const float* c2ws, float near_, float far_,
                        const float* rgb_pool, float* origins, float* directions, float* viewdirs, float* radii,
                        float* lossmult, float* near_out, float* far_out, float* noise_var, float* rgb_out, void* stream) {
    if (B <= 0 || n_cam <= 0 || H <= 0 || W < 3) return PN_ERR_BAD_SHAPE;
    const RayOut out{origins, directions, viewdirs, radii, lossmult, near_out, far_out, noise_var, rgb_out};
    if (!ray_ptrs_ok(idx, c2ws, rgb_pool, out)) return PN_ERR_NULL;
    return launch_sample_rays<128>(B, n_cam, PanoCams{H, W, c2ws}, idx, near_, far_, rgb_pool, out, stream);
}

int pn_sample_pinhole_rays(int64_t B, int n_cam, int H, int W, const int64_t* idx, const float* pix2cams,
                           const float* c2ws, float near_, float far_, const float* rgb_pool, float* origins,
                           float* directions, float* viewdirs, float* radii, float* lossmult, float* near_out,
                           float* far_out, float* noise_var, float* rgb_out, void* stream) {
    if (B <= 0 || n_cam <= 0 || H < 2 || W < 2 || (int64_t)H * W >= ((int64_t)1 << 31)) return PN_ERR_BAD_SHAPE;
    const RayOut out{origins, directions, viewdirs, radii, lossmult, near_out, far_out, noise_var, rgb_out};
    if (!pix2cams || !ray_ptrs_ok(idx, c2ws, rgb_pool, out)) return PN_ERR_NULL;
    return launch_sample_rays<kThreads>(B, n_cam, PinholeCams{H, W, pix2cams, c2ws}, idx, near_, far_, rgb_pool, out, stream);
}

int pn_sample_camera_rays(int64_t B, int n_cam, int kind, int H, int W, const float* params_host, const int64_t* idx,
                          const float* c2ws, float near_, float far_, const float* rgb_pool, float* origins,
                          float* directions, float* viewdirs, float* radii, float* lossmult, float* near_out,
                          float* far_out, float* noise_var, float* rgb_out, void* stream) {
    if (kind != PN_CAM_CUBE && kind != PN_CAM_FISHEYE && kind != PN_CAM_STEREO_PANO) return PN_ERR_UNSUPPORTED;
    bool ok = false;
    min_size(kind, H, W, ok);
    if (B <= 0 || n_cam <= 0 || !ok || (int64_t)H * W >= ((int64_t)1 << 31)) return PN_ERR_BAD_SHAPE;
    const RayOut out{origins, directions, viewdirs, radii, lossmult, near_out, far_out, noise_var, rgb_out};
    if (!params_host || !ray_ptrs_ok(idx, c2ws, rgb_pool, out)) return PN_ERR_NULL;
    const float* p = params_host;
    if (kind == PN_CAM_FISHEYE && !(p[0] > 0.f && p[1] > 0.f)) return PN_ERR_BAD_SHAPE;
    switch (kind) {
        case PN_CAM_CUBE:
            return launch_sample_rays<kThreads>(B, n_cam, CubeCams{H, W, c2ws}, idx, near_, far_, rgb_pool, out, stream);
        case PN_CAM_FISHEYE:
            return launch_sample_rays<kThreads>(B, n_cam, FisheyeCams{H, W, c2ws, p[0], p[1]}, idx, near_, far_, rgb_pool,
                                                out, stream);
        default:
            return launch_sample_rays<kThreads>(B, n_cam, StereoPanoCams{H, W, c2ws, p[0]}, idx, near_, far_, rgb_pool, out,
                                                stream);
    }
}

int pn_reproject(int N, int C, int src_kind, int Hs, int Ws, const float* src_params_host, int dst_kind, int Hd, int Wd,
                 const float* dst_params_host, const float* rotation_host, int samples, float fill, const float* image,
                 int64_t image_stride, int64_t cs, int64_t ps, float* out, float* coverage, void* stream) {
    bool oks = false, okd = false;
    if (!min_size(src_kind, Hs, Ws, oks) || !min_size(dst_kind, Hd, Wd, okd)) return PN_ERR_UNSUPPORTED;
    if (src_kind == PN_CAM_STEREO_PANO || dst_kind == PN_CAM_STEREO_PANO) return PN_ERR_UNSUPPORTED;  // not central
    if (N <= 0 || C <= 0 || !oks || !okd || samples <= 0 || samples > PN_REPROJECT_MAX_SAMPLES ||
        (int64_t)Hs * Ws >= ((int64_t)1 << 31) || (int64_t)Hd * Wd >= ((int64_t)1 << 31))
        return PN_ERR_BAD_SHAPE;
    if (!src_params_host || !dst_params_host || !rotation_host || !image || !out || !coverage) return PN_ERR_NULL;
    if (src_kind == PN_CAM_FISHEYE && !(src_params_host[0] > 0.f && src_params_host[1] > 0.f)) return PN_ERR_BAD_SHAPE;
    if (dst_kind == PN_CAM_FISHEYE && !(dst_params_host[0] > 0.f && dst_params_host[1] > 0.f)) return PN_ERR_BAD_SHAPE;
    CamParams sp, dp;
    Rot rot;
    for (int k = 0; k < PN_CAM_PARAMS; ++k) sp.v[k] = src_params_host[k], dp.v[k] = dst_params_host[k];
    for (int k = 0; k < 9; ++k) rot.m[k] = rotation_host[k];
    const dim3 grid(nblk((int64_t)Hd * Wd, kThreads), (unsigned)(N < 65535 ? N : 65535));
    hipLaunchKernelGGL(k_reproject, grid, dim3(kThreads), 0, ST(stream), N, C, src_kind, Hs, Ws, sp, dst_kind, Hd, Wd, dp,
                       rot, samples, fill, image, image_stride, cs, ps, out, coverage);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_warp_splat(int S, int src_kind, int Hs, int Ws, const float* src_params_host, const float* depth,
                  const float* src_c2ws, int D, int dst_kind, int Hd, int Wd, const float* dst_params_host,
                  const float* dst_c2ws, int max_splat, float scale, uint64_t* zbuf, void* stream) {
    bool oks = false, okd = false;
    if (!min_size(src_kind, Hs, Ws, oks) || !min_size(dst_kind, Hd, Wd, okd)) return PN_ERR_UNSUPPORTED;
    if (src_kind == PN_CAM_STEREO_PANO || dst_kind == PN_CAM_STEREO_PANO) return PN_ERR_UNSUPPORTED;  // not central
    if (S <= 0 || D <= 0 || !oks || !okd || max_splat < 1 || max_splat > PN_WARP_MAX_SPLAT || !(scale > 0.f) ||
        !(scale < INFINITY) || (int64_t)S * Hs * Ws >= ((int64_t)1 << 32) || (int64_t)D * Hd * Wd >= ((int64_t)1 << 31))
        return PN_ERR_BAD_SHAPE;
    if (!src_params_host || !dst_params_host || !depth || !src_c2ws || !dst_c2ws || !zbuf) return PN_ERR_NULL;
    if (src_kind == PN_CAM_FISHEYE && !(src_params_host[0] > 0.f && src_params_host[1] > 0.f)) return PN_ERR_BAD_SHAPE;
    if (dst_kind == PN_CAM_FISHEYE && !(dst_params_host[0] > 0.f && dst_params_host[1] > 0.f)) return PN_ERR_BAD_SHAPE;
    CamParams sp, dp;
    for (int k = 0; k < PN_CAM_PARAMS; ++k) sp.v[k] = src_params_host[k], dp.v[k] = dst_params_host[k];
    const int64_t n_src = (int64_t)S * Hs * Ws;
    const dim3 grid(nblk(n_src, kThreads), (unsigned)(D < 65535 ? D : 65535));
    hipLaunchKernelGGL(k_warp_splat, grid, dim3(kThreads), 0, ST(stream), n_src, src_kind, Hs, Ws, sp, depth, src_c2ws, D,
                       dst_kind, Hd, Wd, dp, dst_c2ws, max_splat, scale, (unsigned long long*)zbuf);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_warp_resolve(int S, int C, int Hs, int Ws, int D, int dst_kind, int Hd, int Wd, const float* dst_params_host,
                    const uint64_t* zbuf, const float* image, int64_t image_stride, int64_t cs, int64_t ps, float fill,
                    float* out, float* depth_out, int64_t* index, float* coverage, void* stream) {
    bool okd = false;
    if (!min_size(dst_kind, Hd, Wd, okd)) return PN_ERR_UNSUPPORTED;
    if (dst_kind == PN_CAM_STEREO_PANO) return PN_ERR_UNSUPPORTED;
    if (S <= 0 || D <= 0 || Hs <= 0 || Ws <= 0 || !okd || (int64_t)S * Hs * Ws >= ((int64_t)1 << 32) ||
        (int64_t)D * Hd * Wd >= ((int64_t)1 << 31) || ((image || out) && C <= 0))
        return PN_ERR_BAD_SHAPE;
    if (!dst_params_host || !zbuf || !depth_out || !index || !coverage || (image == nullptr) != (out == nullptr))
        return PN_ERR_NULL;
    CamParams dp;
    for (int k = 0; k < PN_CAM_PARAMS; ++k) dp.v[k] = dst_params_host[k];
    const int64_t n_dst = (int64_t)D * Hd * Wd;
    hipLaunchKernelGGL(k_warp_resolve, dim3(nblk(n_dst, kThreads)), dim3(kThreads), 0, ST(stream), (int64_t)S * Hs * Ws, C, Hs,
                       Ws, n_dst, dst_kind, Hd, Wd, dp, (const unsigned long long*)zbuf, image, image_stride, cs, ps, fill, out,
                       depth_out, index, coverage);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_warp_blend(int S, int D, int C, int H, int W, const float* images, const float* depths, const float* weights,
                  float depth_ratio, float fill, float* out, float* depth_out, float* coverage, void* stream) {
    if (S <= 0 || D <= 0 || C <= 0 || H <= 0 || W <= 0 || !(depth_ratio >= 0.f && depth_ratio < 1.f) ||
        (int64_t)S * D * C * H * W >= ((int64_t)1 << 31))
        return PN_ERR_BAD_SHAPE;
    if (!images || !depths || !weights || !out || !depth_out || !coverage) return PN_ERR_NULL;
    const int64_t hw = (int64_t)H * W;
    hipLaunchKernelGGL(k_warp_blend, dim3(nblk(D * hw, kThreads)), dim3(kThreads), 0, ST(stream), S, (int64_t)D, C, hw, images,
                       depths, weights, 1.f - depth_ratio, fill, out, depth_out, coverage);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
