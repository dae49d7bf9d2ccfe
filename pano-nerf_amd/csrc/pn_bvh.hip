// pn_bvh.hip — a linear BVH over a mesh's triangles, built on the device (gfx950): the opt-in fast path of virtual object
// insertion.  The contract (padded triangle boxes, the node layout and the depth bound) is stated in
// include/panonerf_hip.h; pn_bvh_walk.h reads and walks the rows, under pn_objects.hip, pn_meshdist.hip and pn_winding.hip.
//
// Build: padded boxes -> 63-bit Morton keys -> (the caller's stable sort) -> Karras' radix tree, one thread per internal
// node -> bottom-up refit, one thread per leaf.  One triangle per leaf; a node row carries both children's boxes, so one
// 64-byte fetch tests both.
#include "pn_bvh_walk.h"
#include "pn_common.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float fmin3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float fmax3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

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
    for (int level = 0; level < pn_bvh::kDepth && cur >= 0 && cur < F - 1; ++level) {
        float* row = nodes + (int64_t)cur * 16;
        const bool left = ((const int32_t*)row)[3] == me;  // written by k_bvh_tree, an earlier launch
        float* mine = row + (left ? 0 : 8);
        const float* other = row + (left ? 8 : 0);
        agent_put(mine, lo.x), agent_put(mine + 1, lo.y), agent_put(mine + 2, lo.z);
        agent_put(mine + 4, hi.x), agent_put(mine + 5, hi.y), agent_put(mine + 6, hi.z);
        __threadfence();
        if (atomicAdd(counters + cur, 1) == 0) return;
        __threadfence();
        lo.x = fminf(lo.x, agent_get(other)), lo.y = fminf(lo.y, agent_get(other + 1)), lo.z = fminf(lo.z, agent_get(other + 2));
        hi.x = fmaxf(hi.x, agent_get(other + 4)), hi.y = fmaxf(hi.y, agent_get(other + 5)), hi.z = fmaxf(hi.z, agent_get(other + 6));
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

}  // namespace

extern "C" {

int pn_bvh_boxes(int64_t F, int64_t V, const float* vertices, const int32_t* faces, float* tbox, void* stream) {
    if (F <= 0 || !count_ok(F) || V < 0) return PN_ERR_BAD_SHAPE;
    if (!faces || !tbox || (V > 0 && !vertices)) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_bvh_boxes, dim3(nblk(F, kThreads)), dim3(kThreads), 0, ST(stream), F, V, vertices, faces,
                       (float4*)tbox);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_bvh_keys(int64_t F, const float* tbox, const float* scene_box, int64_t* keys, void* stream) {
    if (F <= 0 || !count_ok(F)) return PN_ERR_BAD_SHAPE;
    if (!tbox || !scene_box || !keys) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_bvh_keys, dim3(nblk(F, kThreads)), dim3(kThreads), 0, ST(stream), F, (const float4*)tbox,
                       scene_box, keys);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_bvh_tree(int64_t F, const int64_t* sorted_keys, const int64_t* order, const float* tbox, float* nodes,
                int32_t* leaf_parent, int32_t* counters, void* stream) {
    if (F <= 0 || !count_ok(F)) return PN_ERR_BAD_SHAPE;
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

}  // extern "C"
