// pn_winding.hip — generalized winding numbers of a triangle mesh at arbitrary 3-D points (gfx950): the exact sum of the
// triangles' signed solid angles by brute force through LDS tiles, the dipole moments of every node of pn_bvh.hip's tree,
// and a pre-order walk of that tree that replaces far nodes by their dipole (Barnes-Hut).  The contract (the solid angle
// operation for operation, the moments, the opening rule, the order of the sum) is stated in include/panonerf_hip.h,
// section "winding number"; tests/_winding_ref.py restates it in numpy.
#include "pn_common.h"
#include "pn_mesh64.h"
#include "pn_tri.h"
#include <math.h>

namespace {

using pn_tri::kDepth;
using pn_mesh64::P3;
using pn_mesh64::sub3;
using pn_mesh64::dot3;
using pn_mesh64::cross3;
using pn_mesh64::load_tri;  // false: the face contributes nothing

__device__ __forceinline__ P3 add3(const P3 a, const P3 b) { return P3{a.x + b.x, a.y + b.y, a.z + b.z}; }

// Omega(p, f), van Oosterom and Strackee (1983), in the header's order of operations.  num == 0 (p in the face's plane,
// on an edge or on a corner) is the principal value 0: a signed zero never decides between +2 pi and -2 pi.
__device__ __forceinline__ double solid_angle(const P3 p, const P3 a, const P3 b, const P3 c) {
    const P3 A = sub3(a, p), B = sub3(b, p), C = sub3(c, p);
    const double num = dot3(A, cross3(B, C));
    if (num == 0.0) return 0.0;
    const double la = sqrt(dot3(A, A)), lb = sqrt(dot3(B, B)), lc = sqrt(dot3(C, C));
    const double den = ((la * lb) * lc + dot3(A, B) * lc) + (dot3(B, C) * la + dot3(C, A) * lb);
    return 2.0 * atan2(num, den);
}

// the point of thread r, and whether it is asked (every coordinate finite)
__device__ __forceinline__ bool load_point(int64_t r, int64_t P, const float* points, P3& p) {
    p = P3{0.0, 0.0, 0.0};
    if (r >= P) return false;
    const float x = points[r * 3], y = points[r * 3 + 1], z = points[r * 3 + 2];
    p = P3{(double)x, (double)y, (double)z};
    return isfinite(x) && isfinite(y) && isfinite(z);
}

__device__ __forceinline__ float finish(bool ask, double S) { return ask ? (float)(S / PN_WINDING_FOUR_PI) : NAN; }

// ---------------------------------------------------------------------------------------------------------- brute force
// Every face in ascending index, staged through LDS in tiles of kTile corners (3 float4 each, .w of the first = valid:
// 12 KB), as pn_meshdist.hip's BruteNear; S takes the terms in that order.
constexpr int kBruteThreads = 256;
constexpr int kTile = PN_WINDING_TILE;

__global__ __launch_bounds__(kBruteThreads) void k_winding(int64_t P, const float* points, int64_t V, const float* vertices,
                                                          int64_t F, const int32_t* faces, float* winding) {
    __shared__ float4 s_tri[kTile * 3];
    const int64_t r = (int64_t)blockIdx.x * kBruteThreads + threadIdx.x;
    P3 p;
    const bool ask = load_point(r, P, points, p);
    double S = 0.0;
    for (int64_t base = 0; base < F; base += kTile) {
        const int cnt = (int)((F - base) < kTile ? (F - base) : kTile);
        __syncthreads();  // every reader of the previous tile is done
        for (int i = threadIdx.x; i < cnt; i += kBruteThreads) {
            P3 a{0, 0, 0}, b{0, 0, 0}, c{0, 0, 0};
            const bool ok = load_tri(base + i, V, vertices, faces, a, b, c);
            s_tri[i * 3] = make_float4((float)a.x, (float)a.y, (float)a.z, ok ? 1.f : 0.f);
            s_tri[i * 3 + 1] = make_float4((float)b.x, (float)b.y, (float)b.z, 0.f);
            s_tri[i * 3 + 2] = make_float4((float)c.x, (float)c.y, (float)c.z, 0.f);
        }
        __syncthreads();
        if (!ask) continue;
        for (int j = 0; j < cnt; ++j) {
            const float4 a = s_tri[j * 3], b = s_tri[j * 3 + 1], c = s_tri[j * 3 + 2];
            if (a.w == 0.f) continue;
            S += solid_angle(p, P3{a.x, a.y, a.z}, P3{b.x, b.y, b.z}, P3{c.x, c.y, c.z});
        }
    }
    if (r < P) winding[r] = finish(ask, S);
}

// -------------------------------------------------------------------------------------------------------------- moments
// Words of a moments row that another workgroup wrote in this launch are read and written with agent-scope accesses, as
// the box words of pn_bvh.hip's refit are.
__device__ __forceinline__ void put(double* p, double v) {
    __hip_atomic_store((long long*)p, __double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double get(const double* p) {
    return __longlong_as_double(__hip_atomic_load((const long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

struct Part {  // what a child hands to its parent: zero for a face that is not valid and for an empty node
    P3 g, N;
    double A;
};

__device__ __forceinline__ Part child_part(int32_t ref, int64_t F, int64_t V, const float* vertices, const int32_t* faces,
                                           const double* moments) {
    Part q{P3{0.0, 0.0, 0.0}, P3{0.0, 0.0, 0.0}, 0.0};
    if (ref < 0) {
        const int64_t f = ~ref;
        P3 a, b, c;
        if (f < F && load_tri(f, V, vertices, faces, a, b, c)) {  // PN_BVH_NONE gives f = 2^31 - 1 >= F
            const P3 n = cross3(sub3(b, a), sub3(c, a));
            q.N = P3{0.5 * n.x, 0.5 * n.y, 0.5 * n.z};
            q.A = sqrt(dot3(q.N, q.N));
            const P3 s = add3(add3(a, b), c);
            q.g = P3{s.x / 3.0, s.y / 3.0, s.z / 3.0};
        }
    } else if (ref < F - 1) {
        const double* m = moments + (int64_t)ref * 8;
        q.g = P3{get(m), get(m + 1), get(m + 2)};
        q.N = P3{get(m + 4), get(m + 5), get(m + 6)};
        q.A = get(m + 7);
    }
    return q;
}

// the row of internal node i from its two children, left with right in that order
__device__ __forceinline__ void node_row(int64_t i, int64_t F, int64_t V, const float* vertices, const int32_t* faces,
                                         const float4* nodes, double* moments) {
    const float4 a = nodes[i * 4], b = nodes[i * 4 + 1], c = nodes[i * 4 + 2], e = nodes[i * 4 + 3];
    const Part l = child_part(__float_as_int(a.w), F, V, vertices, faces, moments);
    const Part r = child_part(__float_as_int(b.w), F, V, vertices, faces, moments);
    const float lx = fminf(a.x, c.x), ly = fminf(a.y, c.y), lz = fminf(a.z, c.z);
    const float hx = fmaxf(b.x, e.x), hy = fmaxf(b.y, e.y), hz = fmaxf(b.z, e.z);
    double* m = moments + i * 8;
    if (!(lx <= hx)) {  // the empty box: nothing valid below
        for (int k = 0; k < 8; ++k) put(m + k, 0.0);
        return;
    }
    const P3 N = add3(l.N, r.N);
    const double A = l.A + r.A;
    P3 g;
    if (A > 0.0)
        g = P3{(l.A * l.g.x + r.A * r.g.x) / A, (l.A * l.g.y + r.A * r.g.y) / A, (l.A * l.g.z + r.A * r.g.z) / A};
    else
        g = P3{((double)lx + (double)hx) * 0.5, ((double)ly + (double)hy) * 0.5, ((double)lz + (double)hz) * 0.5};
    const double ex = fmax(g.x - (double)lx, (double)hx - g.x), ey = fmax(g.y - (double)ly, (double)hy - g.y),
                 ez = fmax(g.z - (double)lz, (double)hz - g.z);
    put(m, g.x), put(m + 1, g.y), put(m + 2, g.z), put(m + 3, (ex * ex + ey * ey) + ez * ez);
    put(m + 4, N.x), put(m + 5, N.y), put(m + 6, N.z), put(m + 7, A);
}

// One thread per internal node.  A node's row can be written once both children are known: a leaf child is known from
// the start (its quantities are recomputed from the face), an internal child once its own row is written.  The thread of
// node i arrives at i once for its leaf children; a thread that has written a row arrives at the parent.  An arrival that
// completes a node (the second one, or the only one of a node with two leaves) writes its row and goes on; the other
// stops.  Rows are written once, from the same operands in the same order, whoever arrives last.
__global__ __launch_bounds__(256) void k_bvh_moments(int64_t F, int64_t V, const float* vertices, const int32_t* faces,
                                                    const float4* nodes, double* moments, int32_t* counters) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= F - 1) return;
    const int leaves = (__float_as_int(nodes[i * 4].w) < 0) + (__float_as_int(nodes[i * 4 + 1].w) < 0);
    if (leaves == 0) return;
    int64_t cur = i;
    if (leaves == 1) {
        if (atomicAdd(counters + cur, 1) == 0) return;
        __threadfence();
    }
    for (int level = 0; level < kDepth; ++level) {
        node_row(cur, F, V, vertices, faces, nodes, moments);
        const int32_t parent = __float_as_int(nodes[cur * 4 + 2].w);
        if (parent < 0 || parent >= F - 1) return;  // the root, or a row this library did not write
        __threadfence();
        if (atomicAdd(counters + parent, 1) == 0) return;
        __threadfence();
        cur = parent;
    }
}

__global__ void k_zero_row(double* moments) {
    if (threadIdx.x < 8 && blockIdx.x == 0) moments[threadIdx.x] = 0.0;
}

// ------------------------------------------------------------------------------------------------------------ BVH walk
// Pre-order from row 0, the left child first and the right one pushed; S takes the terms in visiting order.  `visits`
// counts every reference taken up, leaf or node, and ends the walk at 2 F: a tree has 2 F - 1 of them, so the bound only
// shows over a buffer that is no tree.
constexpr int kWalkThreads = 64;  // one wave per workgroup: the [depth][thread] stack of pn_tri.h's BvhFinder

__global__ __launch_bounds__(kWalkThreads) void k_winding_bvh(int64_t P, const float* points, int64_t V,
                                                             const float* vertices, int64_t F, const int32_t* faces,
                                                             const float4* nodes, const double* moments, double beta2,
                                                             float* winding) {
    __shared__ int s_stack[kDepth * kWalkThreads];
    int* stack = s_stack + threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    if (r >= P) return;  // no barrier below
    P3 p;
    const bool ask = load_point(r, P, points, p);
    double S = 0.0;
    if (ask) {
        int32_t cur = F > 1 ? 0 : ~0;  // F = 1: the single leaf
        int sp = 0;
        for (int64_t visits = 0; visits < 2 * F; ++visits) {
            if (cur >= 0 && cur < F - 1) {
                const double* m = moments + (int64_t)cur * 8;
                const P3 x = sub3(P3{m[0], m[1], m[2]}, p);
                const double d2 = dot3(x, x);
                if (d2 > 0.0 && d2 >= beta2 * m[3]) {
                    S += dot3(P3{m[4], m[5], m[6]}, x) / (d2 * sqrt(d2));
                } else {
                    const int32_t lref = __float_as_int(nodes[(int64_t)cur * 4].w),
                                  rref = __float_as_int(nodes[(int64_t)cur * 4 + 1].w);
                    if (sp < kDepth) stack[sp++ * kWalkThreads] = rref;  // sp < kDepth always: the depth bound
                    cur = lref;
                    continue;
                }
            } else if (cur < 0) {
                const int64_t f = ~cur;
                P3 a, b, c;
                if (f < F && load_tri(f, V, vertices, faces, a, b, c)) S += solid_angle(p, a, b, c);
            }
            if (sp == 0) break;
            cur = stack[--sp * kWalkThreads];
        }
    }
    winding[r] = finish(ask, S);
}

bool count_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }

}  // namespace

extern "C" {

int pn_winding(int64_t P, const float* points, int64_t V, const float* vertices, int64_t F, const int32_t* faces,
               float* winding, void* stream) {
    if (P < 0 || !count_ok(V) || !count_ok(F)) return PN_ERR_BAD_SHAPE;
    if (P == 0) return PN_OK;
    if (!points || !winding || (F > 0 && !faces) || (F > 0 && V > 0 && !vertices)) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_winding, dim3(nblk(P, kBruteThreads)), dim3(kBruteThreads), 0, ST(stream), P, points, V, vertices,
                       F, faces, winding);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_bvh_moments(int64_t F, int64_t V, const float* vertices, const int32_t* faces, const float* nodes, double* moments,
                   int32_t* counters, void* stream) {
    if (F <= 0 || !count_ok(F) || !count_ok(V)) return PN_ERR_BAD_SHAPE;
    if (!faces || !nodes || !moments || (V > 0 && !vertices)) return PN_ERR_NULL;
    if (F == 1) {
        hipLaunchKernelGGL(k_zero_row, dim3(1), dim3(64), 0, ST(stream), moments);
        PN_CHECK_LAUNCH();
        return PN_OK;
    }
    if (!counters) return PN_ERR_NULL;
    if (hipMemsetAsync(counters, 0, (size_t)(F - 1) * sizeof(int32_t), ST(stream)) != hipSuccess) return PN_ERR_HIP;
    hipLaunchKernelGGL(k_bvh_moments, dim3(nblk(F - 1, 256)), dim3(256), 0, ST(stream), F, V, vertices, faces,
                       (const float4*)nodes, moments, counters);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_winding_bvh(int64_t P, const float* points, int64_t V, const float* vertices, int64_t F, const int32_t* faces,
                   const float* nodes, const double* moments, float beta, float* winding, void* stream) {
    if (P < 0 || !count_ok(V) || !count_ok(F) || F <= 0) return PN_ERR_BAD_SHAPE;  // no tree without a face
    if (!(beta >= 1.f && beta <= 1e6f)) return PN_ERR_BAD_SHAPE;
    if (P == 0) return PN_OK;
    if (!points || !winding || !faces || !nodes || !moments || (V > 0 && !vertices)) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_winding_bvh, dim3(nblk(P, kWalkThreads)), dim3(kWalkThreads), 0, ST(stream), P, points, V,
                       vertices, F, faces, (const float4*)nodes, moments, (double)beta * (double)beta, winding);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
