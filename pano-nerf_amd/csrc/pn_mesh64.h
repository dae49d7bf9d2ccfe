// pn_mesh64.h — the fp64 vector arithmetic, the face and point loaders and the LDS tile that the queries against a mesh share
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

// the point of thread r, and whether it is asked (r < P and every coordinate finite)
__device__ __forceinline__ bool load_point(int64_t r, int64_t P, const float* points, P3& p) {
    p = P3{0.0, 0.0, 0.0};
    if (r >= P) return false;
    const float x = points[r * 3], y = points[r * 3 + 1], z = points[r * 3 + 2];
    p = P3{(double)x, (double)y, (double)z};
    return isfinite(x) && isfinite(y) && isfinite(z);
}

// The brute-force tile: kTile faces in ascending index as 3 float4 of corners each, .w of the first = valid: 12 KB.
// stage_tile, called by EVERY thread of the workgroup in uniform control flow, fills it with the cnt faces from base on.
constexpr int kTile = 256;
template <int kThreads>
__device__ __forceinline__ void stage_tile(int64_t base, int cnt, int64_t V, const float* vertices, const int32_t* faces,
                                           float4* s_tri) {
    __syncthreads();  // every reader of the previous tile is done
    for (int i = threadIdx.x; i < cnt; i += kThreads) {
        P3 a{0, 0, 0}, b{0, 0, 0}, c{0, 0, 0};
        const bool ok = load_tri(base + i, V, vertices, faces, a, b, c);
        s_tri[i * 3] = make_float4((float)a.x, (float)a.y, (float)a.z, ok ? 1.f : 0.f);
        s_tri[i * 3 + 1] = make_float4((float)b.x, (float)b.y, (float)b.z, 0.f);
        s_tri[i * 3 + 2] = make_float4((float)c.x, (float)c.y, (float)c.z, 0.f);
    }
    __syncthreads();
}

// face j of the tile, widened again; false: the face contributes nothing
__device__ __forceinline__ bool tile_tri(const float4* s_tri, int j, P3& a, P3& b, P3& c) {
    const float4 ta = s_tri[j * 3], tb = s_tri[j * 3 + 1], tc = s_tri[j * 3 + 2];
    a = P3{ta.x, ta.y, ta.z}, b = P3{tb.x, tb.y, tb.z}, c = P3{tc.x, tc.y, tc.z};
    return ta.w != 0.f;
}

}  // namespace pn_mesh64
