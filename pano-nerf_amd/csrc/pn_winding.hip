// pn_winding.hip — generalized winding numbers of a triangle mesh at arbitrary 3-D points (gfx950): the exact sum of the
// triangles' signed solid angles by brute force through LDS tiles, the dipole moments of every node of pn_bvh.hip's tree,
// and a pre-order walk of that tree that replaces far nodes by their dipole (Barnes-Hut).  The contract (the solid angle
// operation for operation, the moments, the opening rule, the order of the sum) is stated in include/panonerf_hip.h,
// section "winding number"; tests/_winding_ref.py restates it in numpy.
#include "pn_bvh_walk.h"
#include "pn_common.h"
#include "pn_mesh64.h"
#include <math.h>

namespace {

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

__device__ __forceinline__ float finish(bool ask, double S) { return ask ? (float)(S / PN_WINDING_FOUR_PI) : NAN; }

// ---------------------------------------------------------------------------------------------------------- brute force
// Every face in ascending index through pn_mesh64.h's tile; S takes the terms in that order.
static_assert(PN_WINDING_TILE == pn_mesh64::kTile, "k_winding stages pn_mesh64.h's tile");
constexpr int kBruteThreads = 256;
using pn_mesh64::kTile;

__global__ __launch_bounds__(kBruteThreads) void k_winding(int64_t P, const float* points, int64_t V, const float* vertices,
                                                          int64_t F, const int32_t* faces, float* winding) {
    __shared__ float4 s_tri[kTile * 3];
    const int64_t r = (int64_t)blockIdx.x * kBruteThreads + threadIdx.x;
    P3 p;
    const bool ask = pn_mesh64::load_point(r, P, points, p);
    double S = 0.0;
    for (int64_t base = 0; base < F; base += kTile) {
        const int cnt = (int)((F - base) < kTile ? (F - base) : kTile);
        pn_mesh64::stage_tile<kBruteThreads>(base, cnt, V, vertices, faces, s_tri);
        if (!ask) continue;
        for (int j = 0; j < cnt; ++j) {
            const float4 a = s_tri[j * 3], b = s_tri[j * 3 + 1], c = s_tri[j * 3 + 2];  // pn_mesh64::tile_tri, restated:
            if (a.w == 0.f) continue;                                                   // through it the sum is 2.5 % slower
            S += solid_angle(p, P3{a.x, a.y, a.z}, P3{b.x, b.y, b.z}, P3{c.x, c.y, c.z});
        }
    }
    if (r < P) winding[r] = finish(ask, S);
}

// -------------------------------------------------------------------------------------------------------------- moments
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
        q.g = P3{agent_get(m), agent_get(m + 1), agent_get(m + 2)};
        q.N = P3{agent_get(m + 4), agent_get(m + 5), agent_get(m + 6)};
        q.A = agent_get(m + 7);
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
        for (int k = 0; k < 8; ++k) agent_put(m + k, 0.0);
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
    agent_put(m, g.x), agent_put(m + 1, g.y), agent_put(m + 2, g.z), agent_put(m + 3, (ex * ex + ey * ey) + ez * ez);
    agent_put(m + 4, N.x), agent_put(m + 5, N.y), agent_put(m + 6, N.z), agent_put(m + 7, A);
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
    for (int level = 0; level < pn_bvh::kDepth; ++level) {
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
constexpr int kWalkThreads = 64;  // one wave per workgroup (the LDS stack is per thread)

__global__ __launch_bounds__(kWalkThreads) void k_winding_bvh(int64_t P, const float* points, int64_t V,
                                                             const float* vertices, int64_t F, const int32_t* faces,
                                                             const float4* nodes, const double* moments, double beta2,
                                                             float* winding) {
    __shared__ pn_bvh::Stack<kWalkThreads>::Shared s_stack;
    pn_bvh::Stack<kWalkThreads> stack(s_stack);
    const int64_t r = (int64_t)blockIdx.x * kWalkThreads + threadIdx.x;
    if (r >= P) return;  // no barrier below
    P3 p;
    const bool ask = pn_mesh64::load_point(r, P, points, p);
    double S = 0.0;
    if (ask) {
        int32_t cur = F > 1 ? 0 : ~0;  // F = 1: the single leaf
        for (int64_t visits = 0; visits < 2 * F; ++visits) {
            if (cur >= 0 && cur < F - 1) {
                const double* m = moments + (int64_t)cur * 8;
                const P3 x = sub3(P3{m[0], m[1], m[2]}, p);
                const double d2 = dot3(x, x);
                if (d2 > 0.0 && d2 >= beta2 * m[3]) {
                    S += dot3(P3{m[4], m[5], m[6]}, x) / (d2 * sqrt(d2));
                } else {
                    const pn_bvh::Row n = pn_bvh::read_row(nodes, cur);  // only .w of a and b is used: the ISA loads two words
                    stack.push(n.rref);
                    cur = n.lref;
                    continue;
                }
            } else if (cur < 0) {
                const int64_t f = ~cur;
                P3 a, b, c;
                if (f < F && load_tri(f, V, vertices, faces, a, b, c)) S += solid_angle(p, a, b, c);
            }
            if (stack.empty()) break;
            cur = stack.pop();
        }
    }
    winding[r] = finish(ask, S);
}

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
