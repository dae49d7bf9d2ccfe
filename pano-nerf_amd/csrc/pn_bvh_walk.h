// pn_bvh_walk.h — the node row of pn_bvh.hip's tree, the stack of a walk in LDS and the one ordered, pruned walk (gfx950),
// under pn_tri.h's BvhFinder (rays) and pn_meshdist.hip's BvhNear (points); pn_winding.hip's pre-order walk prunes nothing and
// keeps its loop, on this reader and stack.  include/panonerf_hip.h states the contract.
#pragma once
#include "pn_common.h"

namespace pn_bvh {

constexpr int kDepth = PN_BVH_MAX_DEPTH;  // stack entries per thread
__device__ __forceinline__ int64_t rows(int64_t F) { return F > 1 ? F - 1 : 1; }  // a reference >= rows is of no tree

// a = (left lo, lref), b = (left hi, rref), c = (right lo, parent), e = (right hi, 0); a reference < 0 is the leaf of face ~ref
struct Row {
    float4 a, b, c, e;
    int32_t lref, rref;
};
__device__ __forceinline__ Row read_row(const float4* nodes, int64_t cur) {
    const float4 a = nodes[cur * 4], b = nodes[cur * 4 + 1];
    return Row{a, b, nodes[cur * 4 + 2], nodes[cur * 4 + 3], __float_as_int(a.w), __float_as_int(b.w)};
}

// One walk's stack in LDS, laid out [depth][thread] - lane l always touches bank l % 32, so a wave's accesses never
// conflict - and sized by the depth bound (94 x 64 threads x 4 B = 24 064 B per workgroup of one wave, no scratch): over
// a tree sp < kDepth always holds, over a buffer that is no tree the guard keeps the writes inside.
template <int kThreads>
struct Stack {
    typedef int Shared[kDepth * kThreads];
    int* col;  // this thread's column, stride kThreads
    int sp = 0;
    __device__ __forceinline__ explicit Stack(Shared& s) : col(s + threadIdx.x) {}
    __device__ __forceinline__ void push(int32_t ref) { if (sp < kDepth) col[sp++ * kThreads] = ref; }
    __device__ __forceinline__ bool empty() const { return sp == 0; }
    __device__ __forceinline__ int32_t pop() { return col[--sp * kThreads]; }  // of a stack that is not empty
};

// The ordered, pruned walk from row 0, one query per thread.  A Query supplies its Bound type (fp32 tn of a ray, fp64 lb
// of a point); bound(lo.xyz, hi.xyz, Bound&): can the box hold an answer, and from which bound on; beyond(Bound): strictly
// beyond the best held; leaf(face, Bound): the candidate rule, then the replacement rule with the query's own tie rule;
// done(): any-hit, the search is over (a constant false compiles out).  A child is skipped only when bound() fails or its
// bound is beyond the best; leaf children are visited at once, the left one first; of two internal children the one with
// the smaller bound is entered first (the left on a tie), the other pushed.  Every internal node is entered at most
// once, so F iterations always suffice: the bound also ends the walk over a buffer that is not a tree.
// The right leaf is re-tested against the best, which the left leaf may just have shrunk.  Skipping it changes no
// output: a leaf whose bound is strictly beyond the best fails the candidate rule (bound <= value) or the replacement rule
// for every value it could produce, and in any-hit mode only face >= 0 is read, which the left leaf has then set.
template <int kThreads, class Query>
__device__ __forceinline__ void walk_ordered(const float4* nodes, int64_t F, Stack<kThreads>& stack, Query& q) {
    int32_t cur = 0;
    for (int64_t it = 0; it < F; ++it) {
        const Row n = read_row(nodes, cur);
        typename Query::Bound bl = 0, br = 0;
        bool hl = q.bound(n.a.x, n.a.y, n.a.z, n.b.x, n.b.y, n.b.z, bl) && !q.beyond(bl);
        bool hr = q.bound(n.c.x, n.c.y, n.c.z, n.e.x, n.e.y, n.e.z, br) && !q.beyond(br);
        if (hl && n.lref < 0) {
            q.leaf(~n.lref, bl);
            hl = false;
        }
        if (hr && n.rref < 0) {
            if (!q.beyond(br)) q.leaf(~n.rref, br);
            hr = false;
        }
        if (q.done()) return;
        hl = hl && n.lref < rows(F) && !q.beyond(bl);
        hr = hr && n.rref < rows(F) && !q.beyond(br);
        if (hl && hr) {
            stack.push(bl <= br ? n.rref : n.lref);
            cur = bl <= br ? n.lref : n.rref;
        } else if (hl) {
            cur = n.lref;
        } else if (hr) {
            cur = n.rref;
        } else {
            if (stack.empty()) return;
            cur = stack.pop();
        }
    }
}

}  // namespace pn_bvh
