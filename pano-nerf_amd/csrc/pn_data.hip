// pn_data.hip — dataset ingest (gfx950): the scanline-planar channel planes of one decoded OpenEXR file
// ([Hs][n_ch][Ws], HALF or FLOAT, channels as stored) -> the [Hs/f, Ws/f, C] fp32 interleaved image the ray pools keep.
// Conventions are stated in include/panonerf_hip.h.
//
// One pass over the source, one launch per file, no LDS and no atomics.  One thread per output pixel: it reads the f
// consecutive source columns of its block with one wide load per row and channel (f <= 4; f / V loads of V elements for a
// larger factor, V = the largest of 4, 2, 1 that divides f), so neighbouring lanes read neighbouring addresses; it loops
// over the f rows and the f columns in index order with one fp32 accumulator per channel (a fixed order: repeated launches
// give the same bits), applies the per-material fix-up of datasets/pano_datasets.py:100-116 to the mean and writes its C
// floats, so a wave's stores cover one contiguous span.  The kernel is bandwidth-trivial (profiles/train_ingest.txt).
#include "pn_common.h"
#include <hip/hip_fp16.h>

namespace {

constexpr int kThreads = 256;

template <typename T, int V>
struct Pack {
    T v[V];
} __attribute__((aligned(sizeof(T) * V)));

__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(__half x) { return __half2float(x); }

struct Ingest {
    int Hs, Ws, n_ch, f, kind, flag, C;
    int ch[3];
    float near_, far_, range;
};

template <typename T, int V>
__global__ __launch_bounds__(kThreads) void k_ingest(Ingest a, const T* __restrict__ src, float* __restrict__ out) {
    const int Wo = a.Ws / a.f;
    const int64_t n_out = (int64_t)(a.Hs / a.f) * Wo;
    const int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (pix >= n_out) return;
    const int yo = (int)(pix / Wo), xo = (int)(pix % Wo);
    const float inv = (float)(a.f * a.f);
    float m[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < a.C; ++c) {
        float acc = 0.f;
        for (int r = 0; r < a.f; ++r) {
            // row (yo f + r) < Hs and columns [xo f, xo f + f) < Ws: f divides both sides (checked on the host)
            const T* row = src + ((int64_t)(yo * a.f + r) * a.n_ch + a.ch[c]) * a.Ws + (int64_t)xo * a.f;
            for (int j = 0; j < a.f; j += V) {
                const Pack<T, V> p = *reinterpret_cast<const Pack<T, V>*>(row + j);
#pragma unroll
                for (int k = 0; k < V; ++k) acc += to_f32(p.v[k]);
            }
        }
        m[c] = acc / inv;
    }
    float* o = out + pix * a.C;
    if (a.kind == PN_INGEST_IMAGE) {
        // np.nan_to_num(nan=0) then np.clip(0, 1000): +-inf end on the bounds
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = m[c];
            o[c] = isnan(v) ? 0.f : (v < 0.f ? 0.f : (v > 1000.f ? 1000.f : v));
        }
    } else if (a.kind == PN_INGEST_ALBEDO) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = m[c];
    } else if (a.kind == PN_INGEST_NORMAL) {
        // x * 2 - 1, then (pano scenes) the right product with R_y(pi) = diag(-1, 1, -1)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = m[c] * 2.f - 1.f;
            o[c] = (a.flag && c != 1) ? -v : v;
        }
    } else {  // PN_INGEST_DEPTH: first channel; normalised: np.clip(d, near, far) (NaN stays), (d - near) / (far - near)
        float d = m[0];
        if (a.flag) {
            d = d < a.near_ ? a.near_ : (d > a.far_ ? a.far_ : d);
            d = (d - a.near_) / a.range;
        }
        o[0] = d;
    }
}

template <typename T>
int launch(const Ingest& a, const void* src, float* out, hipStream_t s) {
    const int64_t n_out = (int64_t)(a.Hs / a.f) * (a.Ws / a.f);
    const dim3 grid((unsigned)((n_out + kThreads - 1) / kThreads)), block(kThreads);
    const T* p = static_cast<const T*>(src);
    // a wide load needs its alignment: Ws and every block start are multiples of f, hence of V; the base must be too
    const bool al16 = ((uintptr_t)src & 15) == 0;
    if (a.f % 4 == 0 && al16) hipLaunchKernelGGL((k_ingest<T, 4>), grid, block, 0, s, a, p, out);
    else if (a.f % 2 == 0 && al16) hipLaunchKernelGGL((k_ingest<T, 2>), grid, block, 0, s, a, p, out);
    else hipLaunchKernelGGL((k_ingest<T, 1>), grid, block, 0, s, a, p, out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_ingest_image(int Hs, int Ws, int n_ch, int is_half, const void* planes, int c0, int c1, int c2, int factor, int kind,
                    int flag, float near_, float far_, float* out, void* stream) {
    if (Hs <= 0 || Ws <= 0 || n_ch <= 0 || factor <= 0 || Hs % factor || Ws % factor ||
        (int64_t)Hs * Ws * n_ch >= ((int64_t)1 << 31))
        return PN_ERR_BAD_SHAPE;
    if (kind < PN_INGEST_IMAGE || kind > PN_INGEST_DEPTH) return PN_ERR_UNSUPPORTED;
    if (!planes || !out) return PN_ERR_NULL;
    Ingest a;
    a.Hs = Hs, a.Ws = Ws, a.n_ch = n_ch, a.f = factor, a.kind = kind, a.flag = flag != 0;
    a.C = kind == PN_INGEST_DEPTH ? 1 : 3;
    a.ch[0] = c0, a.ch[1] = c1, a.ch[2] = c2;
    for (int c = 0; c < a.C; ++c)
        if (a.ch[c] < 0 || a.ch[c] >= n_ch) return PN_ERR_BAD_SHAPE;
    a.near_ = near_, a.far_ = far_, a.range = far_ - near_;
    if (kind == PN_INGEST_DEPTH && a.flag && !(a.range > 0.f)) return PN_ERR_BAD_SHAPE;
    return is_half ? launch<__half>(a, planes, out, ST(stream)) : launch<float>(a, planes, out, ST(stream));
}

}  // extern "C"
