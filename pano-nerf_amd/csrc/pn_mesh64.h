// pn_mesh64.h — the fp64 vector arithmetic and the face loader that the queries against a triangle mesh share
// (pn_meshdist.hip: closest point; pn_winding.hip: winding number).  include/panonerf_hip.h, section "mesh distance",
// states the order of operations: separate operations as written, on the fp32 inputs widened to fp64.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace pn_mesh64 {

struct P3 {
    double x, y, z;
};
__device__ __forceinline__ P3 sub3(const P3 a, const P3 b) { return P3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot3(const P3 a, const P3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ P3 cross3(const P3 u, const P3 w) {
    return P3{u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x};
}

// the corners of face f as fp64; false for a face that is never a candidate (an index outside [0, V), a coordinate that
// is not finite: pn_bvh_boxes' rule for the empty box)
__device__ __forceinline__ bool load_tri(int64_t f, int64_t V, const float* vertices, const int32_t* faces, P3& a, P3& b,
                                         P3& c) {
    const int64_t ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
    if (!(ia >= 0 && ia < V && ib >= 0 && ib < V && ic >= 0 && ic < V)) return false;
    const float *pa = vertices + ia * 3, *pb = vertices + ib * 3, *pc = vertices + ic * 3;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && isfinite(pa[k]) && isfinite(pb[k]) && isfinite(pc[k]);
    a = P3{(double)pa[0], (double)pa[1], (double)pa[2]};
    b = P3{(double)pb[0], (double)pb[1], (double)pb[2]};
    c = P3{(double)pc[0], (double)pc[1], (double)pc[2]};
    return ok;
}

}  // namespace pn_mesh64
