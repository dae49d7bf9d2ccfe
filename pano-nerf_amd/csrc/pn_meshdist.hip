// pn_meshdist.hip — distance queries against a triangle mesh (gfx950): the closest point of the mesh to arbitrary 3-D
// points, by brute force through LDS tiles or by a best-first walk of pn_bvh.hip's tree, and deterministic surface sampling.
// The contract (the point / triangle distance operation for operation, the box bound, the candidate rule, why the tree
// cannot matter, the sampling integers) is stated in include/panonerf_hip.h, section "mesh distance";
// tests/_meshdist_ref.py restates it in numpy.
//
// As pn_objects.hip's k_trace<Finder>: one kernel template, two finders.  A finder is built once per thread from the mesh,
// the nodes and its Shared block in LDS and asked with find(ask, p, h) by EVERY thread of the workgroup in uniform control
// flow (the brute-force finder holds barriers).  h.best comes in as max_distance^2 (or +inf) and h.face as -1.  A search
// keeps (best, face) only; the kernel evaluates the winner once more for the closest point and its barycentrics, which
// gives the same fp64 values as the evaluation that won.
#include "pn_bvh_walk.h"
#include "pn_common.h"
#include "pn_mesh64.h"
#include <math.h>

namespace {

using pn_mesh64::P3;
using pn_mesh64::sub3;
using pn_mesh64::dot3;
using pn_mesh64::cross3;
using pn_mesh64::load_tri;

// s + e t per axis: fl(s + fl(e t))
__device__ __forceinline__ P3 along(const P3 s, const P3 e, double t) { return P3{s.x + e.x * t, s.y + e.y * t, s.z + e.z * t}; }
__device__ __forceinline__ double dist2(const P3 p, const P3 q) {
    const P3 r = sub3(p, q);
    return dot3(r, r);
}

// parameter of the closest point of the segment s .. e (header: "segment"): 0 for a segment of length 0
__device__ __forceinline__ double seg_t(const P3 p, const P3 s, const P3 se) {
    const double L = dot3(se, se);
    if (!(L > 0.0)) return 0.0;
    const double t = dot3(sub3(p, s), se) / L;
    return t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
}

// d2(p, f) with the closest point q and its barycentrics (u, v): q = (1 - u - v) a + u b + v c.  Ericson, "Real-Time
// Collision Detection" 5.1.5, in the header's order of operations.
__device__ __forceinline__ double point_tri(const P3 p, const P3 a, const P3 b, const P3 c, P3& q, double& u, double& v) {
    const P3 ab = sub3(b, a), ac = sub3(c, a);
    const P3 n = cross3(ab, ac);
    if (dot3(n, n) == 0.0) {  // no area: the three edge segments ab, bc, ca, a later one replacing only when nearer
        double t = seg_t(p, a, ab);
        q = along(a, ab, t);
        double d = dist2(p, q);
        u = t, v = 0.0;
        const P3 bc = sub3(c, b);
        t = seg_t(p, b, bc);
        P3 q2 = along(b, bc, t);
        double e = dist2(p, q2);
        if (e < d) d = e, q = q2, u = 1.0 - t, v = t;
        const P3 ca = sub3(a, c);
        t = seg_t(p, c, ca);
        q2 = along(c, ca, t);
        e = dist2(p, q2);
        if (e < d) d = e, q = q2, u = 0.0, v = 1.0 - t;
        return d;
    }
    const P3 ap = sub3(p, a);
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) {  // vertex a
        q = a, u = 0.0, v = 0.0;
        return dist2(p, q);
    }
    const P3 bp = sub3(p, b);
    const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) {  // vertex b
        q = b, u = 1.0, v = 0.0;
        return dist2(p, q);
    }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {  // edge ab
        const double t = d1 / (d1 - d3);
        q = along(a, ab, t), u = t, v = 0.0;
        return dist2(p, q);
    }
    const P3 cp = sub3(p, c);
    const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) {  // vertex c
        q = c, u = 0.0, v = 1.0;
        return dist2(p, q);
    }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {  // edge ac
        const double t = d2 / (d2 - d6);
        q = along(a, ac, t), u = 0.0, v = t;
        return dist2(p, q);
    }
    const double va = d3 * d6 - d5 * d4;
    const double g = d4 - d3, h = d5 - d6;
    if (va <= 0.0 && g >= 0.0 && h >= 0.0) {  // edge bc
        const double t = g / (g + h);
        q = along(b, sub3(c, b), t), u = 1.0 - t, v = t;
        return dist2(p, q);
    }
    const double den = 1.0 / ((va + vb) + vc);  // the interior
    u = vb * den, v = vc * den;
    q = along(along(a, ab, u), ac, v);
    return dist2(p, q);
}

struct Near {
    double best;   // starts at max_distance^2 (or +inf), inclusive
    int32_t face;  // -1: none held
};

// the replacement rule: equal d2 keeps the lowest face index, and the starting value itself is within reach
__device__ __forceinline__ void offer(double d, int32_t f, Near& h) {
    if (d < h.best || (d == h.best && (h.face < 0 || f < h.face))) h.best = d, h.face = f;
}

// ---------------------------------------------------------------------------------------------------------- brute force
// Every face in ascending index through pn_mesh64.h's tile.  Ascending order makes the replacement rule a strict < (plus
// the first face that meets best exactly).
static_assert(PN_MESHDIST_TILE == pn_mesh64::kTile, "BruteNear stages pn_mesh64.h's tile");
struct BruteNear {
    static constexpr int kThreads = 256;
    typedef float4 Shared[PN_MESHDIST_TILE * 3];
    int64_t F, V;
    const float* vertices;
    const int32_t* faces;
    float4* s_tri;

    __device__ __forceinline__ BruteNear(int64_t F, int64_t V, const float* vertices, const int32_t* faces, const float4*,
                                         Shared& s)
        : F(F), V(V), vertices(vertices), faces(faces), s_tri(s) {}

    __device__ __forceinline__ void find(bool ask, const P3 p, Near& h) {
        for (int64_t base = 0; base < F; base += PN_MESHDIST_TILE) {
            const int cnt = (int)((F - base) < PN_MESHDIST_TILE ? (F - base) : PN_MESHDIST_TILE);
            pn_mesh64::stage_tile<kThreads>(base, cnt, V, vertices, faces, s_tri);
            if (!ask) continue;
            for (int j = 0; j < cnt; ++j) {
                P3 a, b, c, q;
                double u, v;
                if (!pn_mesh64::tile_tri(s_tri, j, a, b, c)) continue;
                offer(point_tri(p, a, b, c, q, u, v), (int32_t)(base + j), h);
            }
        }
    }
};

// ------------------------------------------------------------------------------------------------------------ BVH walk
// lb(p, box) (header: "Box bound"): monotone in the box - for a box P that holds a box C, lo_P <= lo_C and hi_P >= hi_C
// give fl(lo_P - p) <= fl(lo_C - p) and fl(p - hi_P) <= fl(p - hi_C) (rounding is monotone), max with 0 keeps that, squares
// of non-negative numbers, sums and the final factor are monotone: lb_P <= lb_C.
__device__ __forceinline__ double box_lb(const P3 p, float lx, float ly, float lz, float hx, float hy, float hz) {
    if (!(lx <= hx)) return INFINITY;  // the empty box
    const double gx = fmax(fmax((double)lx - p.x, 0.0), p.x - (double)hx);
    const double gy = fmax(fmax((double)ly - p.y, 0.0), p.y - (double)hy);
    const double gz = fmax(fmax((double)lz - p.z, 0.0), p.z - (double)hz);
    return ((gx * gx + gy * gy) + gz * gz) * (1.0 - 9.094947017729282e-13);  // 1 - 2^-40
}

struct BvhNear {
    static constexpr int kThreads = 64;  // one wave per workgroup (the LDS stack is per thread)
    using Shared = pn_bvh::Stack<kThreads>::Shared;
    int64_t F, V;
    const float* vertices;
    const int32_t* faces;
    const float4* nodes;
    Shared& shared;

    __device__ __forceinline__ BvhNear(int64_t F, int64_t V, const float* vertices, const int32_t* faces,
                                       const float4* nodes, Shared& s)
        : F(F), V(V), vertices(vertices), faces(faces), nodes(nodes), shared(s) {}

    struct Query {  // pn_bvh::walk_ordered's, of one point
        using Bound = double;  // lb
        const BvhNear& m;
        const P3 p;
        Near& h;
        __device__ __forceinline__ bool bound(float lx, float ly, float lz, float hx, float hy, float hz, double& lb) const {
            lb = box_lb(p, lx, ly, lz, hx, hy, hz);
            return lx <= hx;
        }
        __device__ __forceinline__ bool beyond(double lb) const { return lb > h.best; }
        __device__ __forceinline__ bool done() const { return false; }

        // leaf of face f whose padded box lies lb from p: the candidate rule, then the replacement rule
        __device__ __forceinline__ void leaf(int32_t f, double lb) {
            if (f < 0 || f >= m.F) return;  // PN_BVH_NONE, or a row this library did not write
            P3 a, b, c, q;
            if (!load_tri(f, m.V, m.vertices, m.faces, a, b, c)) return;
            double u, v;
            const double d = point_tri(p, a, b, c, q, u, v);
            if (lb <= d) offer(d, f, h);
        }
    };

    __device__ __forceinline__ void find(bool ask, const P3 p, Near& h) const {
        if (!ask) return;
        pn_bvh::Stack<kThreads> stack(shared);
        Query q{*this, p, h};
        pn_bvh::walk_ordered(nodes, F, stack, q);
    }
};

template <class Finder>
__global__ __launch_bounds__(Finder::kThreads) void k_closest(int64_t P, const float* points, int64_t V,
                                                             const float* vertices, int64_t F, const int32_t* faces,
                                                             const float4* nodes, float max_distance, float* dist_out,
                                                             int32_t* face_out, float* closest_out, float* bary_out) {
    __shared__ typename Finder::Shared s_find;
    const int64_t r = (int64_t)blockIdx.x * Finder::kThreads + threadIdx.x;
    P3 p;
    const bool ask = pn_mesh64::load_point(r, P, points, p);
    Near h{(double)max_distance * (double)max_distance, -1};
    Finder finder(F, V, vertices, faces, nodes, s_find);
    finder.find(ask, p, h);
    if (r >= P) return;
    float d = INFINITY, qx = 0.f, qy = 0.f, qz = 0.f, bu = 0.f, bv = 0.f;
    if (h.face >= 0) {
        P3 a, b, c, q;
        double u, v;
        load_tri(h.face, V, vertices, faces, a, b, c);
        point_tri(p, a, b, c, q, u, v);  // the evaluation that won, once more
        d = (float)sqrt(h.best);
        qx = (float)q.x, qy = (float)q.y, qz = (float)q.z, bu = (float)u, bv = (float)v;
    }
    dist_out[r] = d;
    face_out[r] = h.face;
    closest_out[r * 3] = qx, closest_out[r * 3 + 1] = qy, closest_out[r * 3 + 2] = qz;
    bary_out[r * 2] = bu, bary_out[r * 2 + 1] = bv;
}

// ------------------------------------------------------------------------------------------------------------ sampling
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void k_face_areas(int64_t F, int64_t V, const float* vertices, const int32_t* faces,
                                                        double* area) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    P3 a, b, c;
    double s = 0.0;
    if (load_tri(f, V, vertices, faces, a, b, c)) {
        const P3 n = cross3(sub3(b, a), sub3(c, a));
        s = 0.5 * sqrt(dot3(n, n));
    }
    area[f] = s;
}

__global__ __launch_bounds__(kThreads) void k_face_weights(int64_t F, const double* area, const double* largest,
                                                          int64_t* weight) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const double m = largest[0], s = area[f];
    int64_t w = 0;
    if (m > 0.0 && m < INFINITY && s > 0.0 && s <= m) w = (int64_t)floor(s / m * PN_MESHDIST_WEIGHT_ONE);
    weight[f] = w;
}

__global__ __launch_bounds__(kThreads) void k_sample(int64_t count, int64_t W, int64_t F, int64_t V, const float* vertices,
                                                    const int32_t* faces, const int64_t* cum, float* points,
                                                    int32_t* face_out, float* bary) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const int64_t t = i * (W / count) + i * (W % count) / count;  // floor(i W / count) without the product i W
    int64_t lo = 0, hi = F - 1;  // the first face whose running weight exceeds t
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        if (cum[mid] > t)
            hi = mid;
        else
            lo = mid + 1;
    }
    P3 a, b, c;
    float px = 0.f, py = 0.f, pz = 0.f, bu = 0.f, bv = 0.f;
    int32_t f = -1;
    if (load_tri(lo, V, vertices, faces, a, b, c)) {
        const double x1 = 0.5 + PN_MESHDIST_R2_A1 * (double)i, x2 = 0.5 + PN_MESHDIST_R2_A2 * (double)i;
        double r1 = x1 - floor(x1), r2 = x2 - floor(x2);
        if (r1 + r2 > 1.0) r1 = 1.0 - r1, r2 = 1.0 - r2;
        const P3 q = along(along(a, sub3(b, a), r1), sub3(c, a), r2);
        f = (int32_t)lo;
        px = (float)q.x, py = (float)q.y, pz = (float)q.z, bu = (float)r1, bv = (float)r2;
    }
    points[i * 3] = px, points[i * 3 + 1] = py, points[i * 3 + 2] = pz;
    face_out[i] = f;
    bary[i * 2] = bu, bary[i * 2 + 1] = bv;
}

template <class Finder>
int closest_point(int64_t P, const float* points, int64_t V, const float* vertices, int64_t F, const int32_t* faces,
                  const float* nodes, float max_distance, float* distance, int32_t* face, float* closest, float* bary,
                  void* stream) {
    if (P < 0 || !count_ok(V) || !count_ok(F) || !(max_distance >= 0.f)) return PN_ERR_BAD_SHAPE;
    if (P == 0) return PN_OK;
    if (!points || !distance || !face || !closest || !bary || (F > 0 && !faces) || (F > 0 && V > 0 && !vertices))
        return PN_ERR_NULL;
    hipLaunchKernelGGL(k_closest<Finder>, dim3(nblk(P, Finder::kThreads)), dim3(Finder::kThreads), 0, ST(stream), P, points,
                       V, vertices, F, faces, (const float4*)nodes, max_distance, distance, face, closest, bary);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_closest_point(int64_t P, const float* points, int64_t V, const float* vertices, int64_t F, const int32_t* faces,
                     float max_distance, float* distance, int32_t* face, float* closest, float* bary, void* stream) {
    return closest_point<BruteNear>(P, points, V, vertices, F, faces, nullptr, max_distance, distance, face, closest, bary,
                                    stream);
}

int pn_closest_point_bvh(int64_t P, const float* points, int64_t V, const float* vertices, int64_t F, const int32_t* faces,
                         const float* nodes, float max_distance, float* distance, int32_t* face, float* closest,
                         float* bary, void* stream) {
    if (F <= 0) return PN_ERR_BAD_SHAPE;  // no tree without a face: pn_closest_point answers F = 0
    if (P > 0 && !nodes) return PN_ERR_NULL;
    return closest_point<BvhNear>(P, points, V, vertices, F, faces, nodes, max_distance, distance, face, closest, bary,
                                  stream);
}

int pn_face_areas(int64_t F, int64_t V, const float* vertices, const int32_t* faces, double* area, void* stream) {
    if (!count_ok(F) || !count_ok(V)) return PN_ERR_BAD_SHAPE;
    if (F == 0) return PN_OK;
    if (!faces || !area || (V > 0 && !vertices)) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_face_areas, dim3(nblk(F, kThreads)), dim3(kThreads), 0, ST(stream), F, V, vertices, faces, area);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_face_weights(int64_t F, const double* area, const double* largest, int64_t* weight, void* stream) {
    if (!count_ok(F)) return PN_ERR_BAD_SHAPE;
    if (F == 0) return PN_OK;
    if (!area || !largest || !weight) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_face_weights, dim3(nblk(F, kThreads)), dim3(kThreads), 0, ST(stream), F, area, largest, weight);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_sample_surface(int64_t count, int64_t W, int64_t F, int64_t V, const float* vertices, const int32_t* faces,
                      const int64_t* cum_weight, float* points, int32_t* face, float* bary, void* stream) {
    if (!count_ok(count) || !count_ok(F) || !count_ok(V) || F == 0 || W <= 0 || W > ((int64_t)1 << 62))
        return PN_ERR_BAD_SHAPE;
    if (count == 0) return PN_OK;
    if (!faces || !cum_weight || !points || !face || !bary || (V > 0 && !vertices)) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_sample, dim3(nblk(count, kThreads)), dim3(kThreads), 0, ST(stream), count, W, F, V, vertices,
                       faces, cum_weight, points, face, bary);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
