// pn_atlas.hip — baking the learned scene into textures (gfx950): the per-triangle atlas (UVs, and per texel the owning
// face, its barycentrics, world point, normals and footprint variance), the tangent-space encoding of baked normals in the
// frame pn_texture_hits decodes, and the quantiser of the 8-bit images.  The layout (cells, margins, ownership) is stated
// in include/panonerf_hip.h.
//
// One face / one texel / one value per thread, no LDS, no atomics, no scratch; fp64 on the fp32 inputs, rounded once per
// output: two calls on the same inputs give the same bits.
#include "pn_common.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;

// texel (i, j) of an S x S atlas of c x c cells, n = S / c per row: the owning face (-1: nobody's) and the barycentrics
// (u, v) of the texel's centre in that face's affine map, extrapolated outside the triangle
__device__ __forceinline__ int64_t texel_owner(int i, int j, int c, int n, int64_t F, double& u, double& v) {
    u = v = 0.0;
    if (i >= n * c || j >= n * c) return -1;
    const int row = i / c, col = j / c, li = i - row * c, lj = j - col * c;
    const int h = li + lj + 1 >= c ? 1 : 0;
    const int64_t f = 2 * ((int64_t)row * n + col) + h;
    if (f >= F) return -1;
    const double x = lj + 0.5, y = li + 0.5, L = (double)(c - 2 * PN_ATLAS_MARGIN - PN_ATLAS_DIAG);
    if (h == 0) {
        u = (x - PN_ATLAS_MARGIN) / L, v = (y - PN_ATLAS_MARGIN) / L;
    } else {
        u = ((double)(c - PN_ATLAS_MARGIN) - x) / L, v = ((double)(c - PN_ATLAS_MARGIN) - y) / L;
    }
    return f;
}

__global__ __launch_bounds__(kThreads) void k_atlas_uv(int64_t F, int S, int c, float* uv) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int n = S / c, L = c - 2 * PN_ATLAS_MARGIN - PN_ATLAS_DIAG;
    const int64_t k = f >> 1;
    const int h = (int)(f & 1), row = (int)(k / n), col = (int)(k % n);
    const int a = h ? c - PN_ATLAS_MARGIN : PN_ATLAS_MARGIN, s = h ? -L : L;  // P0 = (a, a), P1 = (a + s, a), P2 = (a, a + s)
    const double X0 = (double)col * c + a, Y0 = (double)row * c + a;
    const double X[3] = {X0, X0 + s, X0}, Y[3] = {Y0, Y0, Y0 + s};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        uv[(f * 3 + q) * 2] = (float)(X[q] / (double)S);
        uv[(f * 3 + q) * 2 + 1] = (float)(1.0 - Y[q] / (double)S);
    }
}

struct TexelArgs {
    int S, c;
    int64_t F, V;
    const float *vertices, *vnormals;
    const int32_t* faces;
    int32_t* face;
    float *bary, *points, *normals_g, *normals_s, *var;
};

__global__ __launch_bounds__(kThreads) void k_atlas_texels(TexelArgs a) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (int64_t)a.S * a.S) return;
    double u, v;
    const int64_t f = texel_owner((int)(t / a.S), (int)(t % a.S), a.c, a.S / a.c, a.F, u, v);
    float bary[2] = {0.f, 0.f}, pt[3] = {0.f, 0.f, 0.f}, ng[3] = {0.f, 0.f, 0.f}, ns[3] = {0.f, 0.f, 0.f}, var = 0.f;
    bool m = f >= 0;
    int64_t i0 = 0, i1 = 0, i2 = 0;
    if (m) {
        i0 = a.faces[f * 3], i1 = a.faces[f * 3 + 1], i2 = a.faces[f * 3 + 2];
        m = i0 >= 0 && i0 < a.V && i1 >= 0 && i1 < a.V && i2 >= 0 && i2 < a.V;
    }
    if (m) {
        const float *p0 = a.vertices + i0 * 3, *p1 = a.vertices + i1 * 3, *p2 = a.vertices + i2 * 3;
        bool finite = true;
#pragma unroll
        for (int q = 0; q < 3; ++q) finite = finite && isfinite(p0[q]) && isfinite(p1[q]) && isfinite(p2[q]);
        if (finite) {
            const double w0 = 1.0 - u - v;
            const double e1[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
            const double e2[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
            const double g[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                                 e1[0] * e2[1] - e1[1] * e2[0]};
            const double A_w = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
            const double L = (double)(a.c - 2 * PN_ATLAS_MARGIN - PN_ATLAS_DIAG);
            bary[0] = (float)u, bary[1] = (float)v;
#pragma unroll
            for (int q = 0; q < 3; ++q) pt[q] = (float)(w0 * p0[q] + u * p1[q] + v * p2[q]);
            if (A_w > 0.0) {
                var = (float)(A_w / (12.0 * L * L));
#pragma unroll
                for (int q = 0; q < 3; ++q) ng[q] = (float)(g[q] / A_w);
                if (a.vnormals) {
                    const float *n0 = a.vnormals + i0 * 3, *n1 = a.vnormals + i1 * 3, *n2 = a.vnormals + i2 * 3;
                    const double nx = w0 * n0[0] + u * n1[0] + v * n2[0], ny = w0 * n0[1] + u * n1[1] + v * n2[1],
                                 nz = w0 * n0[2] + u * n1[2] + v * n2[2];
                    double nn = sqrt(nx * nx + ny * ny + nz * nz);
                    nn = nn < 1e-30 ? 1e-30 : nn;  // as pn_object_hits
                    ns[0] = (float)(nx / nn), ns[1] = (float)(ny / nn), ns[2] = (float)(nz / nn);
                } else {
                    ns[0] = ng[0], ns[1] = ng[1], ns[2] = ng[2];
                }
            }
        }
    }
    a.face[t] = (int32_t)f;
    a.bary[t * 2] = bary[0], a.bary[t * 2 + 1] = bary[1];
    a.var[t] = var;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        a.points[t * 3 + q] = pt[q];
        a.normals_g[t * 3 + q] = ng[q];
        a.normals_s[t * 3 + q] = ns[q];
    }
}

struct EncodeArgs {
    int S;
    int64_t F, V;
    const float *vertices, *uv, *normals_s, *world;
    const int32_t *faces, *face;
    float* out;
};

// m = (n . T', n . B', n . N) in the Gram-Schmidt frame of k_texture_hits (pn_textures.hip), the same expressions in the
// same order; 0.5 m + 0.5 is what that kernel's m = 2 s - 1 undoes
__global__ __launch_bounds__(kThreads) void k_atlas_encode(EncodeArgs a) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (int64_t)a.S * a.S) return;
    float out[3] = {0.5f, 0.5f, 1.f};
    const int64_t f = a.face[t];
    bool ok = f >= 0 && f < a.F;
    int64_t i0 = 0, i1 = 0, i2 = 0;
    if (ok) {
        i0 = a.faces[f * 3], i1 = a.faces[f * 3 + 1], i2 = a.faces[f * 3 + 2];
        ok = i0 >= 0 && i0 < a.V && i1 >= 0 && i1 < a.V && i2 >= 0 && i2 < a.V;
    }
    if (ok) {
        const float* q = a.uv + f * 6;
        const double du1 = (double)q[2] - q[0], dv1 = (double)q[3] - q[1], du2 = (double)q[4] - q[0],
                     dv2 = (double)q[5] - q[1];
        const double det = du1 * dv2 - du2 * dv1;
        const float *p0 = a.vertices + i0 * 3, *p1 = a.vertices + i1 * 3, *p2 = a.vertices + i2 * 3;
        const double N[3] = {a.normals_s[t * 3], a.normals_s[t * 3 + 1], a.normals_s[t * 3 + 2]};
        const double n[3] = {a.world[t * 3], a.world[t * 3 + 1], a.world[t * 3 + 2]};
        ok = det != 0.0 && isfinite(det);
        if (ok) {
            double tt[3], bb[3], Tn[3], Bn[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double e1 = (double)p1[k] - p0[k], e2 = (double)p2[k] - p0[k];
                tt[k] = (e1 * dv2 - e2 * dv1) / det;
                bb[k] = (e2 * du1 - e1 * du2) / det;
            }
            const double nt = N[0] * tt[0] + N[1] * tt[1] + N[2] * tt[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) Tn[k] = tt[k] - N[k] * nt;
            const double tl = sqrt(Tn[0] * Tn[0] + Tn[1] * Tn[1] + Tn[2] * Tn[2]);
            ok = tl >= 1e-12;  // NaN fails
#pragma unroll
            for (int k = 0; k < 3; ++k) Tn[k] /= tl;
            const double nb = N[0] * bb[0] + N[1] * bb[1] + N[2] * bb[2];
            const double tb = Tn[0] * bb[0] + Tn[1] * bb[1] + Tn[2] * bb[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) Bn[k] = bb[k] - N[k] * nb - Tn[k] * tb;
            const double bl = sqrt(Bn[0] * Bn[0] + Bn[1] * Bn[1] + Bn[2] * Bn[2]);
            ok = ok && bl >= 1e-12;
#pragma unroll
            for (int k = 0; k < 3; ++k) Bn[k] /= bl;
            const double mx = n[0] * Tn[0] + n[1] * Tn[1] + n[2] * Tn[2];
            const double my = n[0] * Bn[0] + n[1] * Bn[1] + n[2] * Bn[2];
            const double mz = n[0] * N[0] + n[1] * N[1] + n[2] * N[2];
            ok = ok && isfinite(mx) && isfinite(my) && isfinite(mz) && mz > 0.0;
            if (ok) out[0] = (float)(0.5 * mx + 0.5), out[1] = (float)(0.5 * my + 0.5), out[2] = (float)(0.5 * mz + 0.5);
        }
    }
    a.out[t * 3] = out[0], a.out[t * 3 + 1] = out[1], a.out[t * 3 + 2] = out[2];
}

__global__ __launch_bounds__(kThreads) void k_atlas_quantize(int64_t n, const float* x, const float* table, uint8_t* out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float xf = x[i];
    const double v = !(xf > 0.f) ? 0.0 : (xf > 1.f ? 1.0 : (double)xf);  // NaN -> 0
    int code;
    if (table) {
        int lo = 0, hi = 255;  // the largest code whose value is <= v (table[0] = 0 <= v), then its upper neighbour
#pragma unroll 1
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((double)table[mid] <= v) lo = mid; else hi = mid - 1;
        }
        code = lo;
        if (lo < 255 && (double)table[lo + 1] - v < v - (double)table[lo]) code = lo + 1;  // a tie keeps the lower code
    } else {
        code = (int)rint(255.0 * v);  // round half to even
    }
    out[i] = (uint8_t)code;
}

bool atlas_ok(int S, int c) { return S >= 1 && S <= PN_TEX_MAX_SIZE && c >= PN_ATLAS_MIN_CELL && c <= S; }
bool faces_fit(int64_t F, int S, int c) { return F >= 0 && F <= 2 * (int64_t)(S / c) * (S / c); }

}  // namespace

extern "C" {

int pn_atlas_uv(int64_t F, int S, int c, float* uv, void* stream) {
    if (!atlas_ok(S, c) || !faces_fit(F, S, c)) return PN_ERR_BAD_SHAPE;
    if (F == 0) return PN_OK;
    if (!uv) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_atlas_uv, dim3(nblk(F, kThreads)), dim3(kThreads), 0, ST(stream), F, S, c, uv);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_atlas_texels(int S, int c, int64_t F, int64_t V, const float* vertices, const int32_t* faces,
                    const float* vertex_normals, int32_t* face, float* bary, float* points, float* normals_g,
                    float* normals_s, float* var, void* stream) {
    if (!atlas_ok(S, c) || !faces_fit(F, S, c) || V < 0) return PN_ERR_BAD_SHAPE;
    if (!face || !bary || !points || !normals_g || !normals_s || !var) return PN_ERR_NULL;
    if (F > 0 && (!vertices || !faces)) return PN_ERR_NULL;
    TexelArgs a{S, c, F, V, vertices, vertex_normals, faces, face, bary, points, normals_g, normals_s, var};
    hipLaunchKernelGGL(k_atlas_texels, dim3(nblk((int64_t)S * S, kThreads)), dim3(kThreads), 0, ST(stream), a);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_atlas_encode_normals(int S, int c, int64_t F, int64_t V, const float* vertices, const int32_t* faces,
                            const float* uv, const int32_t* face, const float* normals_s, const float* world_normals,
                            float* out, void* stream) {
    if (!atlas_ok(S, c) || !faces_fit(F, S, c) || V < 0) return PN_ERR_BAD_SHAPE;
    if (!face || !normals_s || !world_normals || !out) return PN_ERR_NULL;
    if (F > 0 && (!vertices || !faces || !uv)) return PN_ERR_NULL;
    EncodeArgs a{S, F, V, vertices, uv, normals_s, world_normals, faces, face, out};
    hipLaunchKernelGGL(k_atlas_encode, dim3(nblk((int64_t)S * S, kThreads)), dim3(kThreads), 0, ST(stream), a);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_atlas_quantize(int64_t count, int C, const float* x, const float* table, uint8_t* out, void* stream) {
    if (count < 0 || C < 1 || C > 4 || count >= ((int64_t)1 << 36)) return PN_ERR_BAD_SHAPE;
    if (count == 0) return PN_OK;
    if (!x || !out) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_atlas_quantize, dim3(nblk(count * C, kThreads)), dim3(kThreads), 0, ST(stream), count * C, x,
                       table, out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
