// pn_tri.h — the ray / triangle test and the bounding-sphere test shared by the brute-force tracer (pn_objects.hip) and
// the BVH tracer (pn_bvh.hip): one definition, the same bits on both paths.
#pragma once
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

}  // namespace pn_tri
