// pn_tri.h — what a mesh tracer asks of the triangles (gfx950): the ray / triangle test, the bounding-sphere test and the
// two finders behind pn_objects.hip's k_trace<Finder> and k_shadow<Finder>, brute force through LDS tiles and a walk of
// pn_bvh.hip's tree.  One definition of each: both paths run the same test on the same rows.
//
// A finder is built once per thread from (F, tris, nodes, its Shared block in LDS) and asked with
//   find(ask, ox, oy, oz, dx, dy, dz, any, h)
// by EVERY thread of the workgroup in uniform control flow (the brute-force finder holds barriers); ask = this thread has
// a ray.  h.best comes in as the ray's t_max (or +inf) and h.face as -1; an accepted hit leaves (best, u, v, face) in h.
// any: the first hit found ends the ray's search, and of h only face means anything.  kThreads is the workgroup size a
// finder is written for.
#pragma once
#include "pn_bvh_walk.h"
#include "pn_common.h"
#include <math.h>

namespace pn_tri {

constexpr float kEdgeEps = PN_OBJ_EDGE_EPS;

// Moeller-Trumbore, two-sided, fp32, separate operations in this order (tests restate it in numpy fp32):
//   p = d x e2, det = e1 . p (0 or NaN: miss), inv = 1 / det, s = o - v0, u = (s . p) inv, q = s x e1, v = (d . q) inv,
//   t = (e2 . q) inv; hit when -eps <= u, -eps <= v, u + v <= 1 + eps and 0 < t < +inf.
__device__ __forceinline__ bool mt_hit(float ox, float oy, float oz, float dx, float dy, float dz, const float4 v0,
                                       const float4 e1, const float4 e2, float& t, float& u, float& v) {
    const float px = dy * e2.z - dz * e2.y, py = dz * e2.x - dx * e2.z, pz = dx * e2.y - dy * e2.x;
    const float det = e1.x * px + e1.y * py + e1.z * pz;
    if (!(det != 0.f)) return false;
    const float inv = 1.f / det;
    const float sx = ox - v0.x, sy = oy - v0.y, sz = oz - v0.z;
    u = (sx * px + sy * py + sz * pz) * inv;
    if (!(u >= -kEdgeEps)) return false;
    const float qx = sy * e1.z - sz * e1.y, qy = sz * e1.x - sx * e1.z, qz = sx * e1.y - sy * e1.x;
    v = (dx * qx + dy * qy + dz * qz) * inv;
    if (!(v >= -kEdgeEps) || !(u + v <= 1.f + kEdgeEps)) return false;
    t = (e2.x * qx + e2.y * qy + e2.z * qz) * inv;
    return t > 0.f && t < INFINITY;
}

// can the ray o + t d (t > 0) reach the sphere bs = (centre, radius)?  fp64, with the radius widened by 0.1 % + 1e-6, so
// that a ray the fp32 test above lets hit a triangle inside the sphere is never turned away.  NaN anywhere: false.
__device__ __forceinline__ bool reaches_sphere(double ox, double oy, double oz, double dx, double dy, double dz,
                                               const float* bs) {
    const double mx = (double)bs[0] - ox, my = (double)bs[1] - oy, mz = (double)bs[2] - oz;
    const double r = (double)bs[3] * 1.001 + 1e-6, r2 = r * r;
    const double mm = mx * mx + my * my + mz * mz;
    if (mm <= r2) return true;  // the origin is inside
    const double b = mx * dx + my * dy + mz * dz, dd = dx * dx + dy * dy + dz * dz;
    return b > 0.0 && mm * dd - b * b <= r2 * dd;
}

struct Hit {
    float best, u, v;  // best starts at t_max (or +inf)
    int32_t face;      // -1: none held
};

// ---------------------------------------------------------------------------------------------------------- brute force
// Every triangle in face order, streamed through LDS in tiles of kTriTile (3 float4 each: 12 KB): a later face replaces
// the best only when its t is smaller, so equal t keeps the lower face index whatever the tile size.  The tile loop ends
// when a vote finds no thread still searching.  A tile that is already in LDS is not staged again: `staged` survives from
// one question to the next (k_shadow asks once per probe pixel, and a mesh of one tile is loaded once).
struct BruteFinder {
    static constexpr int kThreads = 256;
    static constexpr int kTriTile = 256;
    static constexpr bool kNodes = false;
    struct Shared {
        float4 tri[kTriTile * 3];
    };
    int64_t F;
    const float4* tris;
    float4* s_tri;
    int64_t staged = -1;  // base of the triangle tile in LDS (the same in every thread)

    __device__ __forceinline__ BruteFinder(int64_t F, const float4* tris, const float4*, Shared& s)
        : F(F), tris(tris), s_tri(s.tri) {}

    __device__ __forceinline__ void find(bool ask, float ox, float oy, float oz, float dx, float dy, float dz, bool any,
                                         Hit& h) {
        if (!__syncthreads_or(ask)) return;
        for (int64_t base = 0; base < F; base += kTriTile) {
            const int cnt = (int)((F - base) < kTriTile ? (F - base) : kTriTile);
            if (staged != base) {  // every reader of the old tile is past the vote that ended its loop
                for (int i = threadIdx.x; i < cnt * 3; i += kThreads) s_tri[i] = tris[base * 3 + i];
                staged = base;
                __syncthreads();
            }
            if (ask) {
                for (int j = 0; j < cnt; ++j) {
                    float t, u, v;
                    if (mt_hit(ox, oy, oz, dx, dy, dz, s_tri[j * 3], s_tri[j * 3 + 1], s_tri[j * 3 + 2], t, u, v) &&
                        t < h.best) {
                        h.face = (int32_t)(base + j);
                        if (any) {  // best stays what it was: under k_shadow's +inf the compare above folds away
                            ask = false;
                            break;
                        }
                        h.best = t, h.u = u, h.v = v;
                    }
                }
            }
            if (!__syncthreads_or(ask)) break;  // also the barrier before the next tile overwrites this one
        }
    }
};

// ------------------------------------------------------------------------------------------------------------ BVH walk
// include/panonerf_hip.h states the contract; the walk and its stack are pn_bvh_walk.h's.  One ray per thread: neighbours
// ask about neighbouring rays (or the same direction from neighbouring points), so a wave's walks stay close.
constexpr float kShrink = 1.f - 4.76837158203125e-07f;  // 1 - 2^-21
constexpr float kGrow = 1.f + 4.76837158203125e-07f;    // 1 + 2^-21

struct Ray {
    float ox, oy, oz, dx, dy, dz, ix, iy, iz;
    bool sx, sy, sz;  // the axis is a slab: 1 / d is not finite
    bool ok;          // every component of o and d is finite
};

__device__ __forceinline__ Ray make_ray(float ox, float oy, float oz, float dx, float dy, float dz) {
    Ray r;
    r.ox = ox, r.oy = oy, r.oz = oz, r.dx = dx, r.dy = dy, r.dz = dz;
    r.ok = isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(dx) && isfinite(dy) && isfinite(dz);
    r.ix = 1.f / dx, r.iy = 1.f / dy, r.iz = 1.f / dz;
    r.sx = !(fabsf(r.ix) < INFINITY), r.sy = !(fabsf(r.iy) < INFINITY), r.sz = !(fabsf(r.iz) < INFINITY);
    return r;
}

// one axis of the box test: false when the axis alone rules the box out
__device__ __forceinline__ bool axis(float lo, float hi, float o, float inv, bool slab, float& tn, float& tf) {
    if (slab) return lo <= o && o <= hi;
    const float a = (lo - o) * inv, b = (hi - o) * inv;
    tn = fmaxf(tn, fminf(a, b));
    tf = fminf(tf, fmaxf(a, b));
    return true;
}

// Does the ray pass the box [lo, hi], and from which tn on?  (header: "Box test".)
// Monotone in the box: let box P hold box C (lo_P <= lo_C <= hi_C <= hi_P per axis, which exact min / max unions give).
//   * inv finite: x -> fl(x - o) and x -> fl(x inv) are monotone (rounding is), the second rising for inv > 0 and falling
//     for inv < 0, so for inv > 0: a_P <= a_C <= b_C <= b_P, for inv < 0 the mirror image; either way
//     min(a, b)_P <= min(a, b)_C and max(a, b)_P >= max(a, b)_C.  With o and d finite, inv finite and non-zero and lo <= hi,
//     neither a nor b is NaN (no 0 x inf, no inf - inf), so min / max never drop an operand.
//   * slab (d == 0 or 1 / d overflows): lo_C <= o <= hi_C implies lo_P <= o <= hi_P, and near = -inf, far = +inf leave tn
//     and tf alone: P passes the axis whenever C does.
//   * tn = max of the nears, tf = min of the fars: monotone in each.
//   * the outward rounding x -> fl(x c), c = 1 -+ 2^-21 chosen by the sign of x, is monotone on each side of 0, maps
//     x <= 0 to <= 0 and x > 0 to >= 0, hence monotone overall; -inf and +inf stay.
// So tn_P <= tn_C and tf_P >= tf_C, and when C is passed (tn_C <= tf_C, tf_C >= 0) so is P.
__device__ __forceinline__ bool box_pass(const Ray& r, float lx, float ly, float lz, float hx, float hy, float hz, float& tn) {
    if (!r.ok || !(lx <= hx)) return false;  // a ray that is not finite; the empty box
    float n = -INFINITY, f = INFINITY;
    if (!axis(lx, hx, r.ox, r.ix, r.sx, n, f) || !axis(ly, hy, r.oy, r.iy, r.sy, n, f) ||
        !axis(lz, hz, r.oz, r.iz, r.sz, n, f))
        return false;
    n = n > 0.f ? n * kShrink : n * kGrow;
    f = f > 0.f ? f * kGrow : f * kShrink;
    tn = n;
    return n <= f && f >= 0.f;
}

struct BvhFinder {
    static constexpr int kThreads = 64;  // one wave per workgroup (the LDS stack is per thread)
    static constexpr bool kNodes = true;
    using Shared = pn_bvh::Stack<kThreads>::Shared;
    int64_t F;
    const float4 *tris, *nodes;
    Shared& shared;

    __device__ __forceinline__ BvhFinder(int64_t F, const float4* tris, const float4* nodes, Shared& s)
        : F(F), tris(tris), nodes(nodes), shared(s) {}

    template <bool kAny>
    struct Query {  // pn_bvh::walk_ordered's, of one ray
        using Bound = float;  // tn
        const BvhFinder& m;
        const Ray& r;
        Hit& h;
        __device__ __forceinline__ bool bound(float lx, float ly, float lz, float hx, float hy, float hz, float& tn) const {
            return box_pass(r, lx, ly, lz, hx, hy, hz, tn);
        }
        __device__ __forceinline__ bool beyond(float tn) const { return tn > h.best; }
        __device__ __forceinline__ bool done() const { return kAny && h.face >= 0; }

        // leaf of face f, whose padded box the ray passes from tn on: the candidate rule, then the replacement rule
        __device__ __forceinline__ void leaf(int32_t f, float tn) {
            if (f < 0 || f >= m.F) return;  // PN_BVH_NONE, or a row this library did not write
            const float4* tri = m.tris + (int64_t)f * 3;
            float t, u, v;
            if (!mt_hit(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, tri[0], tri[1], tri[2], t, u, v) || !(tn <= t)) return;
            if (t < h.best || (t == h.best && h.face >= 0 && f < h.face)) h.best = t, h.face = f, h.u = u, h.v = v;
        }
    };

    __device__ __forceinline__ void find(bool ask, float ox, float oy, float oz, float dx, float dy, float dz, bool any,
                                         Hit& h) const {
        if (!ask) return;
        pn_bvh::Stack<kThreads> stack(shared);
        const Ray r = make_ray(ox, oy, oz, dx, dy, dz);
        if (any) {
            Query<true> q{*this, r, h};
            pn_bvh::walk_ordered(nodes, F, stack, q);
        } else {
            Query<false> q{*this, r, h};
            pn_bvh::walk_ordered(nodes, F, stack, q);
        }
    }
};

}  // namespace pn_tri
