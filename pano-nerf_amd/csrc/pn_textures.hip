// pn_textures.hip — texture-mapped materials for inserted objects (gfx950): texture ingest (uint8 through a decode table,
// or fp32), the mip pyramid, and the sampler that turns a hit's (face, bary) into albedo, roughness and a tangent-space
// shading normal: UV interpolation, ray-cone level of detail, trilinear filtering, Gram-Schmidt normal mapping.
// Conventions (storage, the footprint, wrap and flip, the fall-backs of the normal map) are stated in
// include/panonerf_hip.h.
//
// One texel / one row per thread, no LDS, no atomics.  The pyramid is fp32 in a fixed order of separate operations (the
// library builds with -ffp-contract=off); the sampler is fp64 on the fp32 inputs, rounded once per output: two calls on the
// same inputs give the same bits, whatever the number of rows per launch.
#include "pn_common.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSize = PN_TEX_MAX_SIZE;

__host__ __device__ inline int lvl(int n, int l) { return (n >> l) > 1 ? (n >> l) : 1; }  // max(1, n >> l)
__host__ __device__ inline int levels(int H, int W) {
    int L = 1;
    for (int m = H > W ? H : W; m > 1; m >>= 1) ++L;
    return L;
}
// texels before level l of an H x W pyramid
__host__ __device__ inline int64_t level_offset(int H, int W, int l) {
    int64_t off = 0;
    for (int i = 0; i < l; ++i) off += (int64_t)lvl(H, i) * lvl(W, i);
    return off;
}

// level 0: texel (y, x) = (image[y, x, 0 .. C-1], 0 ..., alpha); alpha = 1 unless C == 4.  uint8 colour channels go through
// table [256]; a uint8 alpha is fl(i / 255) whatever the table (alpha is never gamma-encoded).
__global__ __launch_bounds__(kThreads) void k_tex_ingest(int64_t n, int C, int is_u8, const void* image,
                                                        const float* table, float4* tex) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    float v[4] = {0.f, 0.f, 0.f, 1.f};
    const uint8_t* p8 = (const uint8_t*)image + i * C;
    const float* p32 = (const float*)image + i * C;
#pragma unroll
    for (int c = 0; c < 4; ++c) {  // unrolled with constant indices: v stays in registers
        if (c >= C) continue;
        if (is_u8)
            v[c] = c == 3 ? (float)((double)p8[c] / 255.0) : table[p8[c]];
        else
            v[c] = p32[c];
    }
    tex[i] = make_float4(v[0], v[1], v[2], v[3]);
}

// dst (y, x) = ((a + b) + (c + d)) * 0.25f of the 2 x 2 block of src, rows and columns clamped to the last one
__global__ __launch_bounds__(kThreads) void k_tex_down(int hs, int ws, int hd, int wd, const float4* src, float4* dst) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (int64_t)hd * wd) return;
    const int y = (int)(i / wd), x = (int)(i % wd);
    const int y0 = 2 * y < hs - 1 ? 2 * y : hs - 1, y1 = 2 * y + 1 < hs - 1 ? 2 * y + 1 : hs - 1;
    const int x0 = 2 * x < ws - 1 ? 2 * x : ws - 1, x1 = 2 * x + 1 < ws - 1 ? 2 * x + 1 : ws - 1;
    const float4 a = src[(int64_t)y0 * ws + x0], b = src[(int64_t)y0 * ws + x1];
    const float4 c = src[(int64_t)y1 * ws + x0], d = src[(int64_t)y1 * ws + x1];
    dst[i] = make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f,
                         ((a.z + b.z) + (c.z + d.z)) * 0.25f, ((a.w + b.w) + (c.w + d.w)) * 0.25f);
}

struct Tex {
    const float4* p;  // NULL: no such map
    int H, W;
};

struct TexHitArgs {
    const uint8_t* mask;
    const int32_t *face, *faces, *face_uv;
    const float *bary, *dirs, *t, *normals_in, *radii, *vertices, *uv;
    int64_t V, F, T;
    Tex tex[3];  // albedo, roughness, normal
    int wrap, flip_v;
    float *albedo, *roughness, *normals, *lod;
};

// texel index i (an integer-valued double) of an axis of n texels: clamped, or wrapped by a non-negative modulo
__device__ __forceinline__ int wrap_index(double i, int n, int wrap) {
    if (wrap) return !(i > 0.0) ? 0 : (i > (double)(n - 1) ? n - 1 : (int)i);  // NaN -> 0: never out of bounds
    if (!(fabs(i) < 9.0e18)) return 0;
    int64_t m = (int64_t)i % n;
    return (int)(m < 0 ? m + n : m);
}

// bilinear sample of level l at (U, V) (V already flipped), channels 0 .. 2
__device__ __forceinline__ void bilinear(const Tex& tx, int l, double U, double V, int wrap, double out[3]) {
    const int h = lvl(tx.H, l), w = lvl(tx.W, l);
    const float4* p = tx.p + level_offset(tx.H, tx.W, l);
    const double x = U * w - 0.5, y = V * h - 0.5;
    const double x0 = floor(x), y0 = floor(y), fx = x - x0, fy = y - y0;
    const int xa = wrap_index(x0, w, wrap), xb = wrap_index(x0 + 1.0, w, wrap);
    const int ya = wrap_index(y0, h, wrap), yb = wrap_index(y0 + 1.0, h, wrap);
    const float4 a00 = p[(int64_t)ya * w + xa], a01 = p[(int64_t)ya * w + xb];
    const float4 a10 = p[(int64_t)yb * w + xa], a11 = p[(int64_t)yb * w + xb];
    out[0] = (1.0 - fy) * ((1.0 - fx) * a00.x + fx * a01.x) + fy * ((1.0 - fx) * a10.x + fx * a11.x);
    out[1] = (1.0 - fy) * ((1.0 - fx) * a00.y + fx * a01.y) + fy * ((1.0 - fx) * a10.y + fx * a11.y);
    out[2] = (1.0 - fy) * ((1.0 - fx) * a00.z + fx * a01.z) + fy * ((1.0 - fx) * a10.z + fx * a11.z);
}

// trilinear sample at level of detail lambda in [0, L - 1].  A whole-numbered lambda reads one level only: the other
// level's weight is 0.
__device__ __forceinline__ void trilinear(const Tex& tx, double lambda, double U, double V, int wrap, double out[3]) {
    const int L = levels(tx.H, tx.W);
    const double fl0 = floor(lambda), f = lambda - fl0;
    const int l0 = (int)fl0, l1 = l0 + 1 < L - 1 ? l0 + 1 : L - 1;
    bilinear(tx, l0, U, V, wrap, out);
    if (f != 0.0) {
        double s1[3];
        bilinear(tx, l1, U, V, wrap, s1);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = (1.0 - f) * out[c] + f * s1[c];
    }
}

__global__ __launch_bounds__(kThreads) void k_texture_hits(int64_t R, TexHitArgs a) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const float n_in[3] = {a.normals_in[r * 3], a.normals_in[r * 3 + 1], a.normals_in[r * 3 + 2]};
    float alb[3] = {0.f, 0.f, 0.f}, rough = 0.f, nrm[3] = {0.f, 0.f, 0.f}, lod[3] = {0.f, 0.f, 0.f};
    const int32_t f = a.face[r];
    bool m = a.mask[r] != 0 && f >= 0 && f < a.F;
    int64_t i0 = 0, i1 = 0, i2 = 0;
    if (m) {
        i0 = a.faces[(int64_t)f * 3], i1 = a.faces[(int64_t)f * 3 + 1], i2 = a.faces[(int64_t)f * 3 + 2];
        m = i0 >= 0 && i0 < a.V && i1 >= 0 && i1 < a.V && i2 >= 0 && i2 < a.V;
    }
    if (m) {
        nrm[0] = n_in[0], nrm[1] = n_in[1], nrm[2] = n_in[2];
        // UVs of the three corners; an index outside [0, T) reads as a non-finite UV
        int64_t j0 = i0, j1 = i1, j2 = i2;
        if (a.face_uv) j0 = a.face_uv[(int64_t)f * 3], j1 = a.face_uv[(int64_t)f * 3 + 1], j2 = a.face_uv[(int64_t)f * 3 + 2];
        const bool uv_ok = j0 >= 0 && j0 < a.T && j1 >= 0 && j1 < a.T && j2 >= 0 && j2 < a.T;
        double u0 = NAN, v0 = NAN, u1 = NAN, v1 = NAN, u2 = NAN, v2 = NAN;
        if (uv_ok) {
            u0 = a.uv[j0 * 2], v0 = a.uv[j0 * 2 + 1];
            u1 = a.uv[j1 * 2], v1 = a.uv[j1 * 2 + 1];
            u2 = a.uv[j2 * 2], v2 = a.uv[j2 * 2 + 1];
        }
        const double bu = a.bary[r * 2], bv = a.bary[r * 2 + 1], w0 = 1.0 - bu - bv;
        const double U = w0 * u0 + bu * u1 + bv * u2;
        double Vt = w0 * v0 + bu * v1 + bv * v2;
        const bool finite_uv = isfinite(U) && isfinite(Vt);
        if (a.flip_v) Vt = 1.0 - Vt;
        const double du1 = u1 - u0, dv1 = v1 - v0, du2 = u2 - u0, dv2 = v2 - v0;
        const double det = du1 * dv2 - du2 * dv1;
        // the triangle and the ray
        const float *p0 = a.vertices + i0 * 3, *p1 = a.vertices + i1 * 3, *p2 = a.vertices + i2 * 3;
        const double e1[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
        const double e2[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
        const double d[3] = {a.dirs[r * 3], a.dirs[r * 3 + 1], a.dirs[r * 3 + 2]};
        const double gx = e1[1] * e2[2] - e1[2] * e2[1], gy = e1[2] * e2[0] - e1[0] * e2[2],
                     gz = e1[0] * e2[1] - e1[1] * e2[0];
        const double A_w = sqrt(gx * gx + gy * gy + gz * gz), A_uv = fabs(det);
        const double dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double c = fabs((gx / A_w) * d[0] + (gy / A_w) * d[1] + (gz / A_w) * d[2]) / dn;
        const double width = a.radii ? 2.0 * (double)a.radii[r] * (double)a.t[r] : 0.0;
        const double lw = log2(width), lc = log2(c);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!a.tex[k].p) continue;
            const Tex tx = a.tex[k];
            double lambda = 0.5 * log2((double)tx.W * (double)tx.H * A_uv / A_w) + lw - lc;
            const double top = (double)(levels(tx.H, tx.W) - 1);
            lambda = lambda > top ? top : (lambda >= 0.0 ? lambda : 0.0);  // NaN -> 0
            lod[k] = (float)lambda;
            double s[3] = {0.0, 0.0, 0.0};
            if (finite_uv) trilinear(tx, lambda, U, Vt, a.wrap, s);
            if (k == 0) {
                alb[0] = (float)s[0], alb[1] = (float)s[1], alb[2] = (float)s[2];
            } else if (k == 1) {
                rough = (float)s[0];
            } else {
                // tangent frame from the UVs, Gram-Schmidt against the shading normal; any failure keeps N
                const double N[3] = {n_in[0], n_in[1], n_in[2]};
                const double mx = 2.0 * s[0] - 1.0, my = 2.0 * s[1] - 1.0, mz = 2.0 * s[2] - 1.0;
                double Tn[3], Bn[3], n[3];
                bool ok = finite_uv && det != 0.0;
                if (ok) {
                    double tt[3], bb[3];
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        tt[q] = (e1[q] * dv2 - e2[q] * dv1) / det;
                        bb[q] = (e2[q] * du1 - e1[q] * du2) / det;
                    }
                    const double nt = N[0] * tt[0] + N[1] * tt[1] + N[2] * tt[2];
#pragma unroll
                    for (int q = 0; q < 3; ++q) Tn[q] = tt[q] - N[q] * nt;
                    const double tl = sqrt(Tn[0] * Tn[0] + Tn[1] * Tn[1] + Tn[2] * Tn[2]);
                    ok = tl >= 1e-12;  // NaN fails
#pragma unroll
                    for (int q = 0; q < 3; ++q) Tn[q] /= tl;
                    const double nb = N[0] * bb[0] + N[1] * bb[1] + N[2] * bb[2];
                    const double tb = Tn[0] * bb[0] + Tn[1] * bb[1] + Tn[2] * bb[2];
#pragma unroll
                    for (int q = 0; q < 3; ++q) Bn[q] = bb[q] - N[q] * nb - Tn[q] * tb;
                    const double bl = sqrt(Bn[0] * Bn[0] + Bn[1] * Bn[1] + Bn[2] * Bn[2]);
                    ok = ok && bl >= 1e-12;
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        Bn[q] /= bl;
                        n[q] = mx * Tn[q] + my * Bn[q] + mz * N[q];
                    }
                    const double nl = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
                    ok = ok && nl >= 1e-12;
#pragma unroll
                    for (int q = 0; q < 3; ++q) n[q] /= nl;
                    ok = ok && isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]);
                    ok = ok && n[0] * d[0] + n[1] * d[1] + n[2] * d[2] < 0.0;  // still facing the eye
                }
                if (ok) nrm[0] = (float)n[0], nrm[1] = (float)n[1], nrm[2] = (float)n[2];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (a.tex[0].p) a.albedo[r * 3 + c] = alb[c];
        if (a.tex[2].p) a.normals[r * 3 + c] = nrm[c];
        if (a.lod) a.lod[r * 3 + c] = lod[c];
    }
    if (a.tex[1].p) a.roughness[r] = rough;
}

bool rows_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31) * kThreads / 2; }
bool size_ok(int H, int W) { return H >= 1 && W >= 1 && H <= kMaxSize && W <= kMaxSize; }

}  // namespace

extern "C" {

int64_t pn_tex_floats(int H, int W) {
    if (!size_ok(H, W)) return PN_ERR_BAD_SHAPE;
    return 4 * level_offset(H, W, levels(H, W));
}

int pn_tex_ingest(int H, int W, int C, int is_u8, const void* image, const float* table, float* tex, void* stream) {
    if (!size_ok(H, W) || C < 1 || C > 4) return PN_ERR_BAD_SHAPE;
    if (!image || !tex || (is_u8 && !table)) return PN_ERR_NULL;
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(k_tex_ingest, dim3(nblk(n, kThreads)), dim3(kThreads), 0, ST(stream), n, C, is_u8 ? 1 : 0, image,
                       table, (float4*)tex);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_tex_pyramid(int H, int W, float* tex, void* stream) {
    if (!size_ok(H, W)) return PN_ERR_BAD_SHAPE;
    if (!tex) return PN_ERR_NULL;
    const int L = levels(H, W);
    float4* src = (float4*)tex;
    for (int l = 0; l + 1 < L; ++l) {
        const int hs = lvl(H, l), ws = lvl(W, l), hd = lvl(H, l + 1), wd = lvl(W, l + 1);
        float4* dst = src + (int64_t)hs * ws;
        hipLaunchKernelGGL(k_tex_down, dim3(nblk((int64_t)hd * wd, kThreads)), dim3(kThreads), 0, ST(stream), hs, ws, hd,
                           wd, (const float4*)src, dst);
        PN_CHECK_LAUNCH();
        src = dst;
    }
    return PN_OK;
}

int pn_texture_hits(int64_t R, const uint8_t* mask, const int32_t* face, const float* bary, const float* directions,
                    const float* t, const float* normals_in, const float* radii, int64_t V, const float* vertices,
                    int64_t F, const int32_t* faces, int64_t T, const float* uv, const int32_t* face_uv,
                    const float* albedo_tex, int albedo_h, int albedo_w, const float* roughness_tex, int roughness_h,
                    int roughness_w, const float* normal_tex, int normal_h, int normal_w, int wrap, int flip_v,
                    float* albedo, float* roughness, float* normals, float* lod, void* stream) {
    if (!rows_ok(R) || V < 0 || F < 0 || T < 0 || F >= ((int64_t)1 << 31)) return PN_ERR_BAD_SHAPE;
    if (wrap != 0 && wrap != 1) return PN_ERR_BAD_SHAPE;
    if ((albedo_tex && !size_ok(albedo_h, albedo_w)) || (roughness_tex && !size_ok(roughness_h, roughness_w)) ||
        (normal_tex && !size_ok(normal_h, normal_w)))
        return PN_ERR_BAD_SHAPE;
    if (R == 0) return PN_OK;
    if (!mask || !face || !bary || !directions || !t || !normals_in) return PN_ERR_NULL;
    if (F > 0 && (!vertices || !faces)) return PN_ERR_NULL;
    if (T > 0 && !uv) return PN_ERR_NULL;
    if ((albedo_tex && !albedo) || (roughness_tex && !roughness) || (normal_tex && !normals)) return PN_ERR_NULL;
    TexHitArgs a{mask, face, faces, face_uv, bary, directions, t, normals_in, radii, vertices, uv, V, F, T,
                 {{(const float4*)albedo_tex, albedo_h, albedo_w},
                  {(const float4*)roughness_tex, roughness_h, roughness_w},
                  {(const float4*)normal_tex, normal_h, normal_w}},
                 wrap ? 1 : 0, flip_v ? 1 : 0, albedo, roughness, normals, lod};
    hipLaunchKernelGGL(k_texture_hits, dim3(nblk(R, kThreads)), dim3(kThreads), 0, ST(stream), R, a);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
