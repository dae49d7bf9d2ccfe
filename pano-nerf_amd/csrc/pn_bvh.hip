// pn_bvh.hip — a linear BVH over a mesh's triangles, built on the device, and the tracers that walk it (gfx950): the
// opt-in fast path of virtual object insertion.  The contract (padded triangle boxes, the box test, the candidate rule,
// why the tree cannot matter, the node layout and the depth bound) is stated in include/panonerf_hip.h; the ray /
// triangle test is pn_tri.h's, the brute-force tracer's own.
//
// Build: padded boxes -> 63-bit Morton keys -> (the caller's stable sort) -> Karras' radix tree, one thread per internal
// node -> bottom-up refit, one thread per leaf.  One triangle per leaf; a node row carries both children's boxes, so one
// 64-byte fetch tests both.  Traversal: one ray (or one scene point) per thread, near child first, the far child pushed
// on a stack in LDS laid out [depth][thread] - lane l always touches bank l % 32, whatever its depth, so a wave's
// accesses never conflict - sized by the depth bound: 94 x 64 threads x 4 B = 24 064 B per workgroup.  No scratch.
#include "pn_common.h"
#include "pn_tri.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;                 // build kernels
constexpr int kWalk = 64;                     // traversal kernels: one wave per workgroup (the LDS stack is per thread)
constexpr int kDepth = PN_BVH_MAX_DEPTH;      // stack entries per thread
constexpr int kTile = 256;                    // probe pixels staged per LDS tile (pn_shadow_ratio_bvh)
constexpr float kShrink = 1.f - 4.76837158203125e-07f;  // 1 - 2^-21
constexpr float kGrow = 1.f + 4.76837158203125e-07f;    // 1 + 2^-21

__device__ __forceinline__ float fmin3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float fmax3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// ---------------------------------------------------------------------------------------------------------------- build
// tbox[f] = (lo - pad, 0), (hi + pad, 0); the empty box (+inf, -inf) for a face that indexes outside [0, V) or has a
// vertex coordinate that is not finite.  pad = fl(fl(REL ext) + fl(ABS mag)).
__global__ __launch_bounds__(kThreads) void k_bvh_boxes(int64_t F, int64_t V, const float* vertices,
                                                       const int32_t* faces, float4* tbox) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V) {
        const float *pa = vertices + a * 3, *pb = vertices + b * 3, *pc = vertices + c * 3;
        const float lx = fmin3(pa[0], pb[0], pc[0]), ly = fmin3(pa[1], pb[1], pc[1]), lz = fmin3(pa[2], pb[2], pc[2]);
        const float hx = fmax3(pa[0], pb[0], pc[0]), hy = fmax3(pa[1], pb[1], pc[1]), hz = fmax3(pa[2], pb[2], pc[2]);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) ok = ok && isfinite(pa[k]) && isfinite(pb[k]) && isfinite(pc[k]);
        if (ok) {
            const float ext = fmax3(hx - lx, hy - ly, hz - lz);
            const float mag = fmax3(fmaxf(fabsf(lx), fabsf(hx)), fmaxf(fabsf(ly), fabsf(hy)), fmaxf(fabsf(lz), fabsf(hz)));
            const float pad = PN_BVH_PAD_REL * ext + PN_BVH_PAD_ABS * mag;
            lo = make_float4(lx - pad, ly - pad, lz - pad, 0.f);
            hi = make_float4(hx + pad, hy + pad, hz + pad, 0.f);
        }
    }
    tbox[f * 2] = lo;
    tbox[f * 2 + 1] = hi;
}

// bits of x (< 2^21) spread to every third position
__device__ __forceinline__ uint64_t spread3(uint64_t x) {
    x &= 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// cell of c within [lo, hi] on a 2^21 grid, fp64; anything out of range or NaN is clamped (the keys only order the
// leaves: any key gives a valid tree)
__device__ __forceinline__ uint64_t cell(float c, float lo, float hi) {
    const double w = (double)hi - (double)lo;
    const double q = w > 0.0 ? ((double)c - (double)lo) / w * 2097152.0 : 0.0;
    if (!(q > 0.0)) return 0;
    return q >= 2097151.0 ? 2097151ull : (uint64_t)q;
}

__global__ __launch_bounds__(kThreads) void k_bvh_keys(int64_t F, const float4* tbox, const float* sb, int64_t* keys) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const float4 lo = tbox[f * 2], hi = tbox[f * 2 + 1];
    int64_t key = 0x7fffffffffffffffll;
    if (lo.x <= hi.x) {
        const uint64_t x = cell(0.5f * lo.x + 0.5f * hi.x, sb[0], sb[3]), y = cell(0.5f * lo.y + 0.5f * hi.y, sb[1], sb[4]),
                       z = cell(0.5f * lo.z + 0.5f * hi.z, sb[2], sb[5]);
        key = (int64_t)(spread3(x) << 2 | spread3(y) << 1 | spread3(z));
    }
    keys[f] = key;
}

// length of the common prefix of (key, position) pairs i and j; -1 outside [0, F).  Keys are < 2^63 and positions
// < 2^31, so the values lie in [1, 63] and [65, 95]: at most 94 of them (PN_BVH_MAX_DEPTH).
__device__ __forceinline__ int prefix(const int64_t* keys, int64_t F, int64_t i, int64_t j) {
    if (j < 0 || j >= F) return -1;
    const uint64_t a = (uint64_t)keys[i], b = (uint64_t)keys[j];
    if (a != b) return __clzll((long long)(a ^ b));
    return 64 + __clz((int)((uint32_t)i ^ (uint32_t)j));
}

// Karras, "Maximizing parallelism in the construction of BVHs, octrees, and k-d trees" (2012), section 3: internal node i
// covers the sorted positions between i and j and splits after position g; a child that covers one position is a leaf.
// Writes the child references and the parents; the boxes come from the refit.
__global__ __launch_bounds__(kThreads) void k_bvh_tree(int64_t F, const int64_t* keys, const int64_t* order, float* nodes,
                                                      int32_t* leaf_parent) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= F - 1) return;
    const int64_t d = prefix(keys, F, i, i + 1) > prefix(keys, F, i, i - 1) ? 1 : -1;
    const int dmin = prefix(keys, F, i, i - d);
    int64_t lmax = 2;
    while (prefix(keys, F, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (prefix(keys, F, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = prefix(keys, F, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (prefix(keys, F, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t first = i < j ? i : j, last = i < j ? j : i;
    if (first == last) return;  // cannot happen with sorted keys; below, first <= g < last keeps every write inside whatever the keys
    int64_t g = i + s * d + (d < 0 ? -1 : 0);
    g = g < first ? first : (g > last - 1 ? last - 1 : g);
    int32_t* row = (int32_t*)(nodes + i * 16);
    if (first == g) {
        row[3] = ~(int32_t)order[g];
        leaf_parent[g] = (int32_t)i;
    } else {
        row[3] = (int32_t)g;
        ((int32_t*)(nodes + g * 16))[11] = (int32_t)i;
    }
    if (last == g + 1) {
        row[7] = ~(int32_t)order[g + 1];
        leaf_parent[g + 1] = (int32_t)i;
    } else {
        row[7] = (int32_t)(g + 1);
        ((int32_t*)(nodes + (g + 1) * 16))[11] = (int32_t)i;
    }
    if (i == 0) row[11] = -1;
    row[15] = 0;
}

// Words of a node row that another workgroup wrote in this launch are read and written with agent-scope accesses, which
// go past the caches that are private to a compute unit or a die.
__device__ __forceinline__ void put(float* p, float v) {
    __hip_atomic_store((int*)p, __float_as_int(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float get(const float* p) {
    return __int_as_float(__hip_atomic_load((const int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// One thread per leaf (sorted position j) climbs towards the root carrying the box of what lies under it.  At a node it
// writes its own side's box, fences and counts its arrival; the first to arrive stops, the second reads the other side,
// takes the union (exact min / max) and goes on.  Each node's box words are written once, by the thread that came up that
// side, so the rows do not depend on who arrived first.
__global__ __launch_bounds__(kThreads) void k_bvh_refit(int64_t F, const int64_t* order, const float4* tbox, float* nodes,
                                                       const int32_t* leaf_parent, int32_t* counters) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= F) return;
    const int64_t face = order[j];
    if (face < 0 || face >= F) return;  // not a permutation: nothing of this library's making
    float4 lo = tbox[face * 2], hi = tbox[face * 2 + 1];
    int32_t me = ~(int32_t)face, cur = leaf_parent[j];
    for (int level = 0; level < kDepth && cur >= 0 && cur < F - 1; ++level) {
        float* row = nodes + (int64_t)cur * 16;
        const bool left = ((const int32_t*)row)[3] == me;  // written by k_bvh_tree, an earlier launch
        float* mine = row + (left ? 0 : 8);
        const float* other = row + (left ? 8 : 0);
        put(mine, lo.x), put(mine + 1, lo.y), put(mine + 2, lo.z);
        put(mine + 4, hi.x), put(mine + 5, hi.y), put(mine + 6, hi.z);
        __threadfence();
        if (atomicAdd(counters + cur, 1) == 0) return;
        __threadfence();
        lo.x = fminf(lo.x, get(other)), lo.y = fminf(lo.y, get(other + 1)), lo.z = fminf(lo.z, get(other + 2));
        hi.x = fmaxf(hi.x, get(other + 4)), hi.y = fmaxf(hi.y, get(other + 5)), hi.z = fmaxf(hi.z, get(other + 6));
        me = cur;
        cur = ((const int32_t*)row)[11];
    }
}

// F = 1: row 0 carries the one leaf on its left and nothing on its right
__global__ void k_bvh_single(const float4* tbox, float4* nodes) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float4 lo = tbox[0], hi = tbox[1];
    nodes[0] = make_float4(lo.x, lo.y, lo.z, __int_as_float(~0));
    nodes[1] = make_float4(hi.x, hi.y, hi.z, __int_as_float(PN_BVH_NONE));
    nodes[2] = make_float4(INFINITY, INFINITY, INFINITY, __int_as_float(-1));
    nodes[3] = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
}

// ------------------------------------------------------------------------------------------------------------ traversal
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

struct Hit {
    float best, u, v;  // best starts at t_max (or +inf)
    int32_t face;      // -1: none held
};

// leaf of face f, whose padded box the ray passes from tn on: the candidate rule, then the replacement rule
__device__ __forceinline__ void leaf(const Ray& r, const float4* tris, int64_t F, int32_t f, float tn, Hit& h) {
    if (f < 0 || f >= F) return;  // PN_BVH_NONE, or a row this library did not write
    float t, u, v;
    if (!pn_tri::mt_hit(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, tris[(int64_t)f * 3], tris[(int64_t)f * 3 + 1],
                        tris[(int64_t)f * 3 + 2], t, u, v))
        return;
    if (!(tn <= t)) return;
    if (t < h.best || (t == h.best && h.face >= 0 && f < h.face)) h.best = t, h.face = f, h.u = u, h.v = v;
}

// Walks the tree from row 0.  A node is skipped only when the ray does not pass its box or tn > best; the near child is
// entered first and the far one pushed.  Every internal node is entered at most once, so F iterations always suffice:
// the bound also ends the walk over a buffer that is not a tree.  stack: this thread's column, stride kWalk.
template <bool kAny>
__device__ __forceinline__ void walk(const Ray& r, int64_t F, const float4* tris, const float4* nodes, int* stack, Hit& h) {
    const int64_t rows = F > 1 ? F - 1 : 1;
    int32_t cur = 0;
    int sp = 0;
    for (int64_t it = 0; it < F; ++it) {
        const float4 a = nodes[(int64_t)cur * 4], b = nodes[(int64_t)cur * 4 + 1], c = nodes[(int64_t)cur * 4 + 2],
                     e = nodes[(int64_t)cur * 4 + 3];
        const int32_t lref = __float_as_int(a.w), rref = __float_as_int(b.w);
        float tl = 0.f, tr = 0.f;
        bool hl = box_pass(r, a.x, a.y, a.z, b.x, b.y, b.z, tl) && !(tl > h.best);
        bool hr = box_pass(r, c.x, c.y, c.z, e.x, e.y, e.z, tr) && !(tr > h.best);
        if (hl && lref < 0) {
            leaf(r, tris, F, ~lref, tl, h);
            hl = false;
        }
        if (hr && rref < 0) {
            leaf(r, tris, F, ~rref, tr, h);
            hr = false;
        }
        if (kAny && h.face >= 0) return;
        hl = hl && lref < rows && !(tl > h.best);
        hr = hr && rref < rows && !(tr > h.best);
        if (hl && hr) {
            const bool left_first = tl <= tr;
            if (sp < kDepth) stack[sp++ * kWalk] = left_first ? rref : lref;  // sp < kDepth always: the depth bound
            cur = left_first ? lref : rref;
        } else if (hl) {
            cur = lref;
        } else if (hr) {
            cur = rref;
        } else {
            if (sp == 0) return;
            cur = stack[--sp * kWalk];
        }
    }
}

__global__ __launch_bounds__(kWalk) void k_trace_bvh(int64_t R, const float* origins, const float* dirs, int64_t F,
                                                    const float4* tris, const float4* nodes, const float* t_max, int any,
                                                    float* t_out, int32_t* face_out, float* bary_out, uint8_t* hit_out) {
    __shared__ int s_stack[kDepth * kWalk];
    const int64_t i = (int64_t)blockIdx.x * kWalk + threadIdx.x;
    if (i >= R) return;
    const Ray r = make_ray(origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2], dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]);
    Hit h{t_max ? t_max[i] : INFINITY, 0.f, 0.f, -1};
    if (any) {
        walk<true>(r, F, tris, nodes, s_stack + threadIdx.x, h);
        hit_out[i] = h.face >= 0;
        return;
    }
    walk<false>(r, F, tris, nodes, s_stack + threadIdx.x, h);
    t_out[i] = h.face >= 0 ? h.best : INFINITY;
    face_out[i] = h.face;
    bary_out[i * 2] = h.face >= 0 ? h.u : 0.f;
    bary_out[i * 2 + 1] = h.face >= 0 ? h.v : 0.f;
}

struct Probe {
    const float* x;
    int64_t cs, ps;  // element (c, pix) at x[c * cs + pix * ps]
};

// pn_objects.hip's k_shadow with the triangle loop replaced by an any-hit walk: one point per thread, the probe's pixels
// in order through LDS, the same fp64 sums in the same order, the same horizon / bounding-sphere early-outs.  Neighbouring
// points ask about the same direction at the same time, so a wave's walks stay close.
__global__ __launch_bounds__(kWalk) void k_shadow_bvh(int64_t R, int64_t HW, Probe pr, const float* dirs,
                                                     const float* omega, const float* points, const float* normals,
                                                     float bias, int64_t F, const float4* tris, const float4* nodes,
                                                     const float* bs, float* out) {
    __shared__ double4 s_dir[kTile];  // l, mean_c L omega
    __shared__ int s_stack[kDepth * kWalk];
    const int64_t r = (int64_t)blockIdx.x * kWalk + threadIdx.x;
    const bool live = r < R;
    float ox = 0.f, oy = 0.f, oz = 0.f;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    bool ok = false;
    if (live) {
        const float px = points[r * 3], py = points[r * 3 + 1], pz = points[r * 3 + 2];
        const float fx = normals[r * 3], fy = normals[r * 3 + 1], fz = normals[r * 3 + 2];
        ok = isfinite(px) && isfinite(py) && isfinite(pz) && isfinite(fx) && isfinite(fy) && isfinite(fz);
        ox = px + bias * fx, oy = py + bias * fy, oz = pz + bias * fz;
        nx = fx, ny = fy, nz = fz;
    }
    bool sees = ok && F > 0;
    if (sees) {  // the whole sphere below the tangent plane: no traced ray (n . l > 0) can reach it
        const double rr = (double)bs[3] * 1.001 + 1e-6;
        const double h = nx * ((double)bs[0] - ox) + ny * ((double)bs[1] - oy) + nz * ((double)bs[2] - oz);
        sees = h + rr * sqrt(nx * nx + ny * ny + nz * nz) > 0.0;
    }
    double e_all = 0.0, e_un = 0.0;
    for (int64_t base = 0; base < HW; base += kTile) {
        const int cnt = (int)((HW - base) < kTile ? (HW - base) : kTile);
        for (int t = threadIdx.x; t < cnt; t += kWalk) {
            const int64_t pix = base + t;
            const float* xp = pr.x + pix * pr.ps;
            const double lm = ((double)xp[0] + (double)xp[pr.cs] + (double)xp[2 * pr.cs]) / 3.0;
            s_dir[t] = make_double4(dirs[pix * 3], dirs[pix * 3 + 1], dirs[pix * 3 + 2], lm * (double)omega[pix]);
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const double4 l = s_dir[t];
            const double c = nx * l.x + ny * l.y + nz * l.z;
            const double wgt = c > 0.0 ? l.w * c : 0.0;
            e_all += wgt;
            bool occ = false;
            if (sees && c > 0.0 && pn_tri::reaches_sphere(ox, oy, oz, l.x, l.y, l.z, bs)) {
                const Ray ray = make_ray(ox, oy, oz, (float)l.x, (float)l.y, (float)l.z);  // exact: the table is fp32
                Hit h{INFINITY, 0.f, 0.f, -1};
                walk<true>(ray, F, tris, nodes, s_stack + threadIdx.x, h);
                occ = h.face >= 0;
            }
            if (!occ) e_un += wgt;
        }
        __syncthreads();
    }
    if (!live) return;
    float ratio = 1.f;
    if (ok && e_all > 0.0) {
        double q = e_un / e_all;
        q = q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);
        if (!isnan(q)) ratio = (float)q;
    }
    out[r] = ratio;
}

bool rows_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31) * kWalk / 2; }
bool faces_ok(int64_t F) { return F > 0 && F < ((int64_t)1 << 31); }

}  // namespace

extern "C" {

int pn_bvh_boxes(int64_t F, int64_t V, const float* vertices, const int32_t* faces, float* tbox, void* stream) {
    if (!faces_ok(F) || V < 0) return PN_ERR_BAD_SHAPE;
    if (!faces || !tbox || (V > 0 && !vertices)) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_bvh_boxes, dim3(nblk(F, kThreads)), dim3(kThreads), 0, ST(stream), F, V, vertices, faces,
                       (float4*)tbox);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_bvh_keys(int64_t F, const float* tbox, const float* scene_box, int64_t* keys, void* stream) {
    if (!faces_ok(F)) return PN_ERR_BAD_SHAPE;
    if (!tbox || !scene_box || !keys) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_bvh_keys, dim3(nblk(F, kThreads)), dim3(kThreads), 0, ST(stream), F, (const float4*)tbox,
                       scene_box, keys);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_bvh_tree(int64_t F, const int64_t* sorted_keys, const int64_t* order, const float* tbox, float* nodes,
                int32_t* leaf_parent, int32_t* counters, void* stream) {
    if (!faces_ok(F)) return PN_ERR_BAD_SHAPE;
    if (!tbox || !nodes) return PN_ERR_NULL;
    if (F == 1) {
        hipLaunchKernelGGL(k_bvh_single, dim3(1), dim3(1), 0, ST(stream), (const float4*)tbox, (float4*)nodes);
        PN_CHECK_LAUNCH();
        return PN_OK;
    }
    if (!sorted_keys || !order || !leaf_parent || !counters) return PN_ERR_NULL;
    if (hipMemsetAsync(counters, 0, (size_t)(F - 1) * sizeof(int32_t), ST(stream)) != hipSuccess) return PN_ERR_HIP;
    hipLaunchKernelGGL(k_bvh_tree, dim3(nblk(F - 1, kThreads)), dim3(kThreads), 0, ST(stream), F, sorted_keys, order,
                       nodes, leaf_parent);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bvh_refit, dim3(nblk(F, kThreads)), dim3(kThreads), 0, ST(stream), F, order,
                       (const float4*)tbox, nodes, leaf_parent, counters);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_trace_mesh_bvh(int64_t R, const float* origins, const float* directions, int64_t F, const float* tris,
                      const float* nodes, const float* t_max, int any_hit, float* t, int32_t* face, float* bary,
                      uint8_t* hit, void* stream) {
    if (!rows_ok(R) || !faces_ok(F)) return PN_ERR_BAD_SHAPE;
    if (R == 0) return PN_OK;
    if (!origins || !directions || !tris || !nodes) return PN_ERR_NULL;
    if (any_hit ? !hit : (!t || !face || !bary)) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_trace_bvh, dim3(nblk(R, kWalk)), dim3(kWalk), 0, ST(stream), R, origins, directions, F,
                       (const float4*)tris, (const float4*)nodes, t_max, any_hit, t, face, bary, hit);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_shadow_ratio_bvh(int64_t R, int H, int W, const float* x, int64_t cs, int64_t ps, const float* dirs,
                        const float* omega, const float* points, const float* normals, float bias, int64_t F,
                        const float* tris, const float* nodes, const float* bsphere, float* out, void* stream) {
    if (!rows_ok(R) || F < 0 || F >= ((int64_t)1 << 31) || H < 2 || W < 2 || (int64_t)H * W >= ((int64_t)1 << 30))
        return PN_ERR_BAD_SHAPE;
    if (R == 0) return PN_OK;
    if (!x || !dirs || !omega || !points || !normals || !out) return PN_ERR_NULL;
    if (F > 0 && (!tris || !nodes || !bsphere)) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_shadow_bvh, dim3(nblk(R, kWalk)), dim3(kWalk), 0, ST(stream), R, (int64_t)H * W,
                       Probe{x, cs, ps}, dirs, omega, points, normals, bias, F, (const float4*)tris,
                       (const float4*)nodes, bsphere, out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
