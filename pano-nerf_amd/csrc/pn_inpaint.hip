// pn_inpaint.hip — depth-aware hole filling of warped frames: push-pull over a pyramid that prefers the background
// (pn_fill_holes, pn_fill_holes_work_floats; the rule is stated in include/panonerf_hip.h).
//
// One thread per texel, looping over the channels; gathers only.  A pull reads level l - 1 and writes level l, a push reads
// level l + 1 and writes the unknown texels of level l, so no launch reads what it writes.  Level 0 is the caller's frame
// (image, depth, known, domain); levels 1 .. L live in the workspace as [N, C + 1, H_l, W_l] planes, z last, z = 0 unknown.
// The small levels would each be a launch of a few hundred texels, i.e. launch latency: k_fill_small runs them in one
// launch, one workgroup per image, planes in LDS (profiles/views_fill.txt: 12 us less per frame).
#include "pn_common.h"

namespace {

constexpr int kThreads = 256;
// k_fill_small takes the levels of at most this many texels (0: every level gets its own launches) ...
#ifndef PN_FILL_SMALL_TEXELS
#define PN_FILL_SMALL_TEXELS 1024
#endif
constexpr int64_t kSmallLdsBytes = 48 << 10;  // ... whose planes together fit into this much LDS

// level 0 as the caller holds it
struct Frame {
    float* image;          // [N, C, H, W]
    float* depth;          // [N, H, W] or NULL (every known pixel has z = 1)
    const float* known;    // [N, H, W], known iff > 0, or NULL (all known)
    const uint8_t* domain; // [H, W] or NULL
    uint8_t* filled;       // [N, H, W]
};

// z of pixel p of image n of the frame: 0 where it is not known
__device__ __forceinline__ float frame_z(const Frame& f, int64_t n, int64_t hw, int64_t p) {
    if (f.domain && !f.domain[p]) return 0.f;
    if (f.known && !(f.known[n * hw + p] > 0.f)) return 0.f;
    if (!f.depth) return 1.f;
    const float z = f.depth[n * hw + p];
    return (z > 0.f && z < INFINITY) ? z : 0.f;
}

// z of a workspace texel: 0 (or anything not positive) is unknown
__device__ __forceinline__ float level_z(const float* lvl, int C, int64_t n, int64_t hw, int64_t p) {
    const float z = lvl[(n * (C + 1) + C) * hw + p];
    return z > 0.f ? z : 0.f;
}

// texel t of image nd of level l (Hd x Wd, planes at dst) from image n of level l - 1 (Hs x Ws: planes at src, or the
// frame when kBase).  src and dst may lie in LDS (k_fill_small), with image 0.
template <bool kBase>
__device__ __forceinline__ void pull_texel(int C, int Hs, int Ws, int Hd, int Wd, float q, const Frame& f, const float* src,
                                           int64_t n, float* dst, int64_t nd, int64_t t) {
    const int64_t hws = (int64_t)Hs * Ws, hwd = (int64_t)Hd * Wd;
    const int y = (int)(t / Wd), x = (int)(t % Wd);
    float z[4];
    int64_t p[4];
    float zf = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = 2 * y + (k >> 1), xx = 2 * x + (k & 1);
        const bool in = yy < Hs && xx < Ws;
        p[k] = in ? (int64_t)yy * Ws + xx : 0;
        z[k] = !in ? 0.f : (kBase ? frame_z(f, n, hws, p[k]) : level_z(src, C, n, hws, p[k]));
        zf = z[k] > zf ? z[k] : zf;
    }
    float* o = dst + nd * (C + 1) * hwd + t;
    if (!(zf > 0.f)) {
        o[(int64_t)C * hwd] = 0.f;
        return;
    }
    const float lim = zf * q;
    bool keep[4];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        keep[k] = z[k] > 0.f && lim <= z[k];
        cnt += keep[k] ? 1 : 0;
    }
    const float fc = (float)cnt;
    for (int c = 0; c <= C; ++c) {
        const float* plane = kBase ? f.image + (n * C + c) * hws : src + (n * (C + 1) + c) * hws;
        float s = 0.f;
        bool first = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!keep[k]) continue;
            const float v = c == C ? z[k] : plane[p[k]];
            s = first ? v : s + v;
            first = false;
        }
        o[(int64_t)c * hwd] = s / fc;
    }
}

// level l (Hd x Wd, workspace) from level l - 1 (Hs x Ws; the frame when kBase)
template <bool kBase>
__global__ __launch_bounds__(kThreads) void k_fill_pull(int64_t total, int C, int Hs, int Ws, int Hd, int Wd, float q, Frame f,
                                                        const float* src, float* dst) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int64_t hwd = (int64_t)Hd * Wd;
    pull_texel<kBase>(C, Hs, Ws, Hd, Wd, q, f, src, idx / hwd, dst, idx / hwd, idx % hwd);
}

// near and far tap of coordinate v of a level in the level above it, of size n: clamped, or wrapped modulo n
__device__ __forceinline__ void taps(int v, int n, bool wrap, int& near_, int& far_) {
    if (v & 1) {
        near_ = (v - 1) >> 1;
        far_ = (v + 1) >> 1;
    } else {
        near_ = v >> 1;
        far_ = (v >> 1) - 1;
    }
    if (wrap) {
        far_ = far_ < 0 ? n - 1 : (far_ >= n ? 0 : far_);
    } else {
        far_ = far_ < 0 ? 0 : (far_ >= n ? n - 1 : far_);
    }
}

// texel t of image nd of level l (Hd x Wd: planes at dst, or the frame when kBase), if it is unknown, from image n of
// level l + 1 (Hs x Ws, planes at src).  src and dst may lie in LDS (k_fill_small), with image 0.
template <bool kBase>
__device__ __forceinline__ void push_texel(int C, int Hd, int Wd, int Hs, int Ws, int wrap_x, float q, const Frame& f,
                                           const float* src, int64_t n, float* dst, int64_t nd, int64_t t) {
    const int64_t hws = (int64_t)Hs * Ws, hwd = (int64_t)Hd * Wd;
    const int64_t idx = nd * hwd + t;
    const int y = (int)(t / Wd), x = (int)(t % Wd);
    if (kBase) {
        f.filled[idx] = 0;
        if (f.domain && !f.domain[t]) return;
        if (frame_z(f, nd, hwd, t) > 0.f) return;
    } else if (level_z(dst, C, nd, hwd, t) > 0.f) {
        return;
    }
    int yn, yf, xn, xf;
    taps(y, Hs, false, yn, yf);
    taps(x, Ws, wrap_x != 0, xn, xf);
    const int64_t p[4] = {(int64_t)yn * Ws + xn, (int64_t)yn * Ws + xf, (int64_t)yf * Ws + xn, (int64_t)yf * Ws + xf};
    const float w[4] = {9.f, 3.f, 3.f, 1.f};
    float z[4];
    float zf = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        z[k] = level_z(src, C, n, hws, p[k]);
        zf = z[k] > zf ? z[k] : zf;
    }
    if (!(zf > 0.f)) return;
    const float lim = zf * q;
    bool keep[4];
    float ws = 0.f;
    bool first = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        keep[k] = z[k] > 0.f && lim <= z[k];
        if (!keep[k]) continue;
        ws = first ? w[k] : ws + w[k];
        first = false;
    }
    for (int c = 0; c <= C; ++c) {
        const float* plane = src + (n * (C + 1) + c) * hws;
        float s = 0.f;
        first = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!keep[k]) continue;
            const float v = w[k] * plane[p[k]];
            s = first ? v : s + v;
            first = false;
        }
        const float v = s / ws;
        if (!kBase) {
            dst[(nd * (C + 1) + c) * hwd + t] = v;
        } else if (c < C) {
            f.image[(nd * C + c) * hwd + t] = v;
        } else if (f.depth) {
            f.depth[idx] = v;
        }
    }
    if (kBase) f.filled[idx] = 1;
}

// the unknown texels of level l (Hd x Wd; the frame when kBase) from level l + 1 (Hs x Ws, workspace)
template <bool kBase>
__global__ __launch_bounds__(kThreads) void k_fill_push(int64_t total, int C, int Hd, int Wd, int Hs, int Ws, int wrap_x, float q,
                                                        Frame f, const float* src, float* dst) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int64_t hwd = (int64_t)Hd * Wd;
    push_texel<kBase>(C, Hd, Wd, Hs, Ws, wrap_x, q, f, src, idx / hwd, dst, idx / hwd, idx % hwd);
}

// size of level j above an Hb x Wb level, and the LDS offset (floats) of its planes behind those of levels 1 .. j - 1
__device__ __forceinline__ void small_level(int Hb, int Wb, int C, int j, int& h, int& w, int& off) {
    h = Hb, w = Wb, off = 0;
    for (int i = 1; i <= j; ++i) {
        if (i > 1) off += (C + 1) * h * w;
        h = (h + 1) >> 1, w = (w + 1) >> 1;
    }
}

// The small levels in one launch: one workgroup per image pulls the `cnt` levels above level b (Hb x Wb: the frame when
// kBase, else the workspace planes at `below`) into LDS, pushes back down through them and then into level b - the
// launches k_fill_pull / k_fill_push would make for those levels, texel for texel, with a barrier for every launch.
template <bool kBase>
__global__ __launch_bounds__(kThreads) void k_fill_small(int C, int Hb, int Wb, int cnt, int wrap_x, float q, Frame f,
                                                         float* below) {
    extern __shared__ float lds[];
    const int64_t n = blockIdx.x;
    int hs = Hb, ws = Wb, hd, wd, os = 0, od;
    for (int j = 1; j <= cnt; ++j) {  // pull level j from level j - 1
        small_level(Hb, Wb, C, j, hd, wd, od);
        for (int t = threadIdx.x; t < hd * wd; t += kThreads) {
            if (j == 1) pull_texel<kBase>(C, hs, ws, hd, wd, q, f, below, n, lds + od, 0, t);
            else pull_texel<false>(C, hs, ws, hd, wd, q, f, lds + os, 0, lds + od, 0, t);
        }
        __syncthreads();
        hs = hd, ws = wd, os = od;
    }
    for (int j = cnt - 1; j >= 0; --j) {  // push level j + 1 into level j
        small_level(Hb, Wb, C, j + 1, hs, ws, os);
        small_level(Hb, Wb, C, j, hd, wd, od);
        for (int t = threadIdx.x; t < hd * wd; t += kThreads) {
            if (j == 0) push_texel<kBase>(C, hd, wd, hs, ws, wrap_x, q, f, lds + os, 0, below, n, t);
            else push_texel<false>(C, hd, wd, hs, ws, wrap_x, q, f, lds + os, 0, lds + od, 0, t);
        }
        __syncthreads();
    }
}

// the number of levels above an H x W frame: up to 1 x 1, or `levels` if that is fewer
int level_count(int H, int W, int levels) {
    int L = 0;
    while ((H > 1 || W > 1) && L < levels) H = (H + 1) >> 1, W = (W + 1) >> 1, ++L;
    return L;
}

bool sizes_ok(int N, int C, int H, int W, int levels) {
    return N > 0 && C > 0 && H > 0 && W > 0 && levels >= 0 && (int64_t)N * (C + 1) * H * W < ((int64_t)1 << 31);
}

int64_t work_floats(int N, int C, int H, int W, int levels) {
    int64_t texels = 0;
    for (int l = level_count(H, W, levels); l > 0; --l) H = (H + 1) >> 1, W = (W + 1) >> 1, texels += (int64_t)H * W;
    return texels * N * (C + 1);
}

}  // namespace

extern "C" {

int64_t pn_fill_holes_work_floats(int N, int C, int H, int W, int levels) {
    if (!sizes_ok(N, C, H, W, levels)) return PN_ERR_BAD_SHAPE;
    return work_floats(N, C, H, W, levels);
}

int pn_fill_holes(int N, int C, int H, int W, float* image, float* depth, const float* known, const uint8_t* domain,
                  int wrap_x, float depth_ratio, int levels, uint8_t* filled, float* work, int64_t work_floats_given,
                  void* stream) {
    if (!sizes_ok(N, C, H, W, levels) || !(depth_ratio >= 0.f && depth_ratio < 1.f)) return PN_ERR_BAD_SHAPE;
    const int L = level_count(H, W, levels);
    if (work_floats_given < work_floats(N, C, H, W, levels)) return PN_ERR_BAD_SHAPE;
    if (!image || !filled || (L > 0 && !work)) return PN_ERR_NULL;
    const float q = 1.f - depth_ratio;
    const Frame f{image, depth, known, domain, filled};
    const hipStream_t s = ST(stream);
    if (L == 0) {  // nothing above the frame: nothing is written
        if (hipMemsetAsync(filled, 0, (size_t)N * H * W, s) != hipSuccess) return PN_ERR_HIP;
        return PN_OK;
    }
    constexpr int kMaxLevels = 32;
    int h[kMaxLevels + 1], w[kMaxLevels + 1];
    float* lvl[kMaxLevels + 1];
    h[0] = H, w[0] = W, lvl[0] = nullptr;
    float* next = work;
    for (int l = 1; l <= L; ++l) {
        h[l] = (h[l - 1] + 1) >> 1, w[l] = (w[l - 1] + 1) >> 1, lvl[l] = next;
        next += (int64_t)N * (C + 1) * h[l] * w[l];
    }
    // levels m .. L, the first whose texels and LDS planes are few enough, run in k_fill_small (m = L + 1: none do)
    int m = L + 1;
    int64_t lds_floats = 0;
    while (m > 1) {
        const int64_t n = (int64_t)h[m - 1] * w[m - 1];
        if (n > PN_FILL_SMALL_TEXELS || (lds_floats + (C + 1) * n) * 4 > kSmallLdsBytes) break;
        lds_floats += (C + 1) * n, --m;
    }
    for (int l = 1; l < m; ++l) {
        const int64_t total = (int64_t)N * h[l] * w[l];
        if (l == 1)
            hipLaunchKernelGGL(k_fill_pull<true>, dim3(nblk(total, kThreads)), dim3(kThreads), 0, s, total, C, h[0], w[0], h[1],
                               w[1], q, f, (const float*)nullptr, lvl[1]);
        else
            hipLaunchKernelGGL(k_fill_pull<false>, dim3(nblk(total, kThreads)), dim3(kThreads), 0, s, total, C, h[l - 1],
                               w[l - 1], h[l], w[l], q, f, (const float*)lvl[l - 1], lvl[l]);
        PN_CHECK_LAUNCH();
    }
    if (m <= L) {
        const size_t lds = (size_t)lds_floats * 4;
        if (m == 1)
            hipLaunchKernelGGL(k_fill_small<true>, dim3(N), dim3(kThreads), lds, s, C, h[0], w[0], L, wrap_x, q, f, (float*)nullptr);
        else
            hipLaunchKernelGGL(k_fill_small<false>, dim3(N), dim3(kThreads), lds, s, C, h[m - 1], w[m - 1], L - m + 1, wrap_x, q,
                               f, lvl[m - 1]);
        PN_CHECK_LAUNCH();
    }
    for (int l = (m <= L ? m - 2 : L - 1); l >= 0; --l) {
        const int64_t total = (int64_t)N * h[l] * w[l];
        if (l == 0)
            hipLaunchKernelGGL(k_fill_push<true>, dim3(nblk(total, kThreads)), dim3(kThreads), 0, s, total, C, h[0], w[0], h[1],
                               w[1], wrap_x, q, f, (const float*)lvl[1], (float*)nullptr);
        else
            hipLaunchKernelGGL(k_fill_push<false>, dim3(nblk(total, kThreads)), dim3(kThreads), 0, s, total, C, h[l], w[l],
                               h[l + 1], w[l + 1], wrap_x, q, f, (const float*)lvl[l + 1], lvl[l]);
        PN_CHECK_LAUNCH();
    }
    return PN_OK;
}

}  // extern "C"
