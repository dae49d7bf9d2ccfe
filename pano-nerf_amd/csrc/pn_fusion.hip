// pn_fusion.hip — TSDF fusion of posed depth images into a signed distance volume (gfx950): per voxel of pn_grid_points'
// grid and per view, the voxel is projected into the view by pn_reproject's inverse projection, the depth of the NEAREST
// pixel is read, and the truncated signed distance along the voxel's own ray is added to a weighted running mean.  The
// formulas are stated term for term in include/panonerf_hip.h.
//
// One voxel per thread with k fastest, so tsdf and weight are read and written coalesced; the views in index order inside
// the kernel, the two fp64 accumulators in registers; the depth image is a gather (neighbouring voxels land on neighbouring
// pixels).  A view's pose is read at a wave-uniform address, so it arrives through the scalar cache once per wave and needs
// no LDS staging and no barrier; the camera parameters are kernel arguments.  One kernel instance per camera kind, so no
// thread carries another kind's projection.  No LDS, no atomics, no scratch; fp64 on the fp32 inputs, every output rounded
// once: two calls on the same inputs give the same bits, whatever the launch geometry.
#include "pn_common.h"
#include "pn_rays.h"

namespace {

constexpr int kThreads = 256;

struct FusionArgs {
    int nx, ny, nz;
    float x0, y0, z0, dx, dy, dz;
    int S, H, W;
    float p[18];  // PINHOLE pix2cam, cam2pix; FISHEYE f, theta_max
    const float *c2ws, *depth, *confidence, *view_weights;
    double trunc;
    float depth_max;
    double max_weight;
    float *tsdf, *weight;
};

// direction e -> the continuous position (qx, qy) of the camera and the cube's face; false where the camera does not see
// it: image_pos<double> (pn_rays.h) written out.  Through the shared template the PINHOLE instance measured 5 % slower (the
// compiler turns its four bounds comparisons into a bit mask there, with kKind under if constexpr too), so this copy stays
// until that is understood
template <int kKind>
__device__ __forceinline__ bool project(const FusionArgs& a, const double e[3], double& qx, double& qy, int& face) {
    face = 0;
    if (kKind == PN_CAM_PANO) {
        const double phi = atan2(hypot(e[0], e[2]), e[1]), theta = atan2(e[0], e[2]);
        double t = -theta / (2.0 * kPiD);
        t = t - floor(t);
        qx = t * (double)a.W;
        qy = phi / kPiD * (double)a.H;
        return true;
    }
    if (kKind == PN_CAM_PINHOLE) {
        double q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            q[k] = ((double)a.p[9 + 3 * k] * e[0] + (double)a.p[10 + 3 * k] * e[1]) + (double)a.p[11 + 3 * k] * e[2];
        if (!(q[2] > 0.0)) return false;
        qx = q[0] / q[2];
        qy = q[1] / q[2];
        return qx >= 0.0 && qx <= (double)a.W && qy >= 0.0 && qy <= (double)a.H;
    }
    if (kKind == PN_CAM_FISHEYE) {
        const double rxy = hypot(e[0], e[1]);
        const double theta = atan2(rxy, -e[2]);
        if (!(theta <= (double)a.p[1])) return false;
        const double r = (double)a.p[0] * theta;
        qx = 0.5 * (double)a.W, qy = 0.5 * (double)a.H;
        if (rxy > 0.0) {
            qx = qx + r * e[0] / rxy;
            qy = qy - r * e[1] / rxy;
        }
        return qx >= 0.0 && qx <= (double)a.W && qy >= 0.0 && qy <= (double)a.H;
    }
    return cube_pos<double>(a.W, e, qx, qy, face);  // qy within the face
}

// min(max(floor q, 0), n - 1); a NaN lands in pixel 0
__device__ __forceinline__ int nearest(double q, int n) {
    const double f = floor(q);
    return f > 0.0 ? (f < (double)(n - 1) ? (int)f : n - 1) : 0;
}

template <int kKind>
__global__ __launch_bounds__(kThreads) void k_tsdf_integrate(FusionArgs a) {
    const int64_t n = (int64_t)a.nx * a.ny * a.nz;
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= n) return;
    const int k = (int)(v % a.nz), j = (int)((v / a.nz) % a.ny), i = (int)(v / ((int64_t)a.nz * a.ny));
    const double X[3] = {(double)a.x0 + (double)i * (double)a.dx, (double)a.y0 + (double)j * (double)a.dy,
                         (double)a.z0 + (double)k * (double)a.dz};
    const int rows = kKind == PN_CAM_CUBE ? a.W : a.H;
    double A = 0.0, B = 0.0;
#pragma unroll 1
    for (int s = 0; s < a.S; ++s) {
        const float* m = a.c2ws + 16 * (int64_t)s;  // wave-uniform: scalar loads
        const double d[3] = {X[0] - (double)m[3], X[1] - (double)m[7], X[2] - (double)m[11]};
        double e[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) e[q] = ((double)m[q] * d[0] + (double)m[4 + q] * d[1]) + (double)m[8 + q] * d[2];  // R^T d
        const double rho = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
        if (!(rho > 0.0 && rho < (double)INFINITY)) continue;
        double qx, qy;
        int face;
        if (!project<kKind>(a, e, qx, qy, face)) continue;
        const int col = nearest(qx, a.W);
        const int row = (kKind == PN_CAM_CUBE ? face * a.W : 0) + nearest(qy, rows);
        const int64_t pix = ((int64_t)s * a.H + row) * a.W + col;
        const float t = a.depth[pix];
        if (!(t > 0.f && t < INFINITY && t <= a.depth_max)) continue;
        double w = a.view_weights ? (double)a.view_weights[s] : 1.0;
        if (a.confidence) w = w * (double)a.confidence[pix];
        if (!(w > 0.0 && w < (double)INFINITY)) continue;
        double z = (double)t;
        if (kKind == PN_CAM_PINHOLE) {  // t runs along pix2cam @ (col + 1/2, row + 1/2, 1), which is not a unit vector
            const double px = (double)col + 0.5, py = (double)row + 0.5;
            double c[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) c[q] = ((double)a.p[3 * q] * px + (double)a.p[3 * q + 1] * py) + (double)a.p[3 * q + 2];
            z = z * sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
        }
        const double sdf = z - rho;
        if (sdf < -a.trunc) continue;  // behind the surface: unseen from this view
        const double q = sdf / a.trunc;
        A = A + w * (q < 1.0 ? q : 1.0);
        B = B + w;
    }
    if (B == 0.0) return;
    const double W0 = (double)a.weight[v];
    const double D0 = W0 == 0.0 ? 0.0 : (double)a.tsdf[v];
    const double W1 = W0 + B;
    a.tsdf[v] = (float)((D0 * W0 + A) / W1);
    a.weight[v] = (float)(W1 < a.max_weight ? W1 : a.max_weight);
}

}  // namespace

extern "C" {

int pn_tsdf_integrate(int nx, int ny, int nz, float x0, float y0, float z0, float dx, float dy, float dz, int S, int kind,
                      int H, int W, const float* params_host, const float* c2ws, const float* depth, const float* confidence,
                      const float* view_weights, float trunc, float depth_max, float max_weight, float* tsdf, float* weight,
                      void* stream) {
    bool ok = false;
    switch (kind) {
        case PN_CAM_PANO: ok = H >= 2 && W >= 3; break;
        case PN_CAM_PINHOLE:
        case PN_CAM_FISHEYE: ok = H >= 2 && W >= 2; break;
        case PN_CAM_CUBE: ok = W >= 2 && (int64_t)H == 6 * (int64_t)W; break;
        default: return PN_ERR_UNSUPPORTED;  // STEREO_PANO is not a central projection
    }
    if (nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny * nz >= ((int64_t)1 << 31) || S <= 0 || !ok ||
        (int64_t)S * H * W >= ((int64_t)1 << 31) || !(trunc > 0.f && trunc < INFINITY) || !(depth_max > 0.f) ||
        !(max_weight > 0.f))
        return PN_ERR_BAD_SHAPE;
    if (!params_host || !c2ws || !depth || !tsdf || !weight) return PN_ERR_NULL;
    if (kind == PN_CAM_FISHEYE && !(params_host[0] > 0.f && params_host[1] > 0.f)) return PN_ERR_BAD_SHAPE;
    FusionArgs a{nx, ny, nz, x0, y0, z0, dx, dy, dz, S, H, W, {}, c2ws, depth, confidence, view_weights,
                 (double)trunc, depth_max, (double)max_weight, tsdf, weight};
    for (int k = 0; k < 18; ++k) a.p[k] = params_host[k];
    const dim3 grid(nblk((int64_t)nx * ny * nz, kThreads)), block(kThreads);
    switch (kind) {
        case PN_CAM_PANO: hipLaunchKernelGGL(k_tsdf_integrate<PN_CAM_PANO>, grid, block, 0, ST(stream), a); break;
        case PN_CAM_PINHOLE: hipLaunchKernelGGL(k_tsdf_integrate<PN_CAM_PINHOLE>, grid, block, 0, ST(stream), a); break;
        case PN_CAM_CUBE: hipLaunchKernelGGL(k_tsdf_integrate<PN_CAM_CUBE>, grid, block, 0, ST(stream), a); break;
        default: hipLaunchKernelGGL(k_tsdf_integrate<PN_CAM_FISHEYE>, grid, block, 0, ST(stream), a); break;
    }
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
