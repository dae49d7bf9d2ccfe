// pn_relight.hip — relighting rendered views with virtual point and spot lights (gfx950): per row (a pixel's ray with its
// depth, normal, albedo and captured colour) and per light, the Lambert / spot / inverse-square term and the visibility
// read from the light's omnidirectional shadow map (a panorama or a cube strip of distances) through a k x k window of
// bilinear depth comparisons.  The formulas are stated term for term in include/panonerf_hip.h.
//
// One row per thread, the lights in index order, no LDS, no atomics, no scratch; fp64 on the fp32 inputs, every output
// rounded once: two calls on the same inputs give the same bits, whatever R.
#include "pn_common.h"
#include "pn_rays.h"

namespace {

constexpr int kThreads = 256;

struct RelightArgs {
    int64_t R;
    const float *origins, *directions, *depth, *normals, *albedo, *rgb;
    int L;
    const float* lights;
    int kind, Hm, Wm;
    const float* maps;
    double ambient, normal_offset, bias_abs, bias_rel, bias_slope;
    int k;
    float *out, *direct, *visibility;
};

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// one bilinear depth comparison at the continuous map position (sx, sy): bilinear_taps<double, int64_t> (pn_rays.h) written
// out, as the panorama branch of k_relight below is image_pos<double>: through the shared templates, though bit-identical,
// k_relight measured 1 % slower at 16 lights, so these copies stay until that is understood
__device__ __forceinline__ double pcf_sample(const float* map, int kind, int Hm, int Wm, int face, double sx, double sy,
                                             double rho, double scale, double bias_abs, double slope) {
    const double gx = sx - 0.5, gy = sy - 0.5;
    const double fx = floor(gx), fy = floor(gy);
    const double wx = gx - fx, wy = gy - fy;
    int64_t x0 = (int64_t)fx, y0 = (int64_t)fy, x1 = x0 + 1, y1 = y0 + 1;
    const int rows = kind == PN_CAM_CUBE ? Wm : Hm;
    if (kind == PN_CAM_PANO) {
        x0 = ((x0 % Wm) + Wm) % Wm;
        x1 = ((x1 % Wm) + Wm) % Wm;
    } else {
        x0 = x0 < 0 ? 0 : (x0 > Wm - 1 ? Wm - 1 : x0);
        x1 = x1 < 0 ? 0 : (x1 > Wm - 1 ? Wm - 1 : x1);
    }
    y0 = y0 < 0 ? 0 : (y0 > rows - 1 ? rows - 1 : y0);
    y1 = y1 < 0 ? 0 : (y1 > rows - 1 ? rows - 1 : y1);
    const int64_t top = kind == PN_CAM_CUBE ? (int64_t)face * Wm : 0;
    const float z[4] = {map[(top + y0) * Wm + x0], map[(top + y0) * Wm + x1], map[(top + y1) * Wm + x0],
                        map[(top + y1) * Wm + x1]};
    double c[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double zq = (double)z[q];
        const bool dark = isfinite(z[q]) && z[q] > 0.f && rho > ((zq * scale + bias_abs) + slope);
        c[q] = dark ? 0.0 : 1.0;
    }
    const double w00 = (1.0 - wy) * (1.0 - wx), w01 = (1.0 - wy) * wx, w10 = wy * (1.0 - wx), w11 = wy * wx;
    return ((w00 * c[0] + w01 * c[1]) + w10 * c[2]) + w11 * c[3];
}

__global__ __launch_bounds__(kThreads) void k_relight(RelightArgs a) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= a.R) return;
    const float tf = a.depth[r];
    bool valid = tf > 0.f && tf < INFINITY;
    double nh[3] = {0.0, 0.0, 0.0};
    if (a.normals) {
        const float* nf = a.normals + r * 3;
        const double n[3] = {nf[0], nf[1], nf[2]};
        const double nn = sqrt(dot3(n, n));
        valid = valid && isfinite(nf[0]) && isfinite(nf[1]) && isfinite(nf[2]) && nn > 1e-12;
        if (valid) nh[0] = n[0] / nn, nh[1] = n[1] / nn, nh[2] = n[2] / nn;
    }
    double X[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) X[q] = (double)a.origins[r * 3 + q] + (double)tf * (double)a.directions[r * 3 + q];
    double E[3] = {0.0, 0.0, 0.0};
    const int k = a.k;
    const int half = (k - 1) / 2;
    const double delta = a.kind == PN_CAM_PANO ? kPiD / (double)a.Hm : 2.0 / (double)a.Wm;
#pragma unroll 1
    for (int li = 0; li < a.L; ++li) {
        const float* lt = a.lights + (int64_t)li * PN_LIGHT_FLOATS;
        double V = 0.0, g = 0.0, r2 = 0.0;
        if (valid) {
            const double p[3] = {lt[0], lt[1], lt[2]};
            const double w[3] = {p[0] - X[0], p[1] - X[1], p[2] - X[2]};
            r2 = dot3(w, w);
            if (r2 > 0.0) {
                const double rr = sqrt(r2);
                const double l[3] = {w[0] / rr, w[1] / rr, w[2] / rr};
                double NoL = 1.0;
                if (a.normals) {
                    const double nl = dot3(nh, l);
                    NoL = nl > 0.0 ? nl : 0.0;
                }
                double spot = 1.0;
                const double ax[3] = {lt[6], lt[7], lt[8]};
                if (!(ax[0] == 0.0 && ax[1] == 0.0 && ax[2] == 0.0)) {
                    const double ci = lt[9], co = lt[10];
                    double s = (-dot3(l, ax) - co) / (ci - co);
                    s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
                    spot = (s * s) * (3.0 - 2.0 * s);
                }
                g = NoL * spot;
                if (g > 0.0) {
                    double v[3];
#pragma unroll
                    for (int q = 0; q < 3; ++q) v[q] = (X[q] + a.normal_offset * nh[q]) - p[q];
                    const double rho = sqrt(dot3(v, v));
                    double qx = 0.0, qy = 0.0;
                    int face = 0;
                    bool seen = rho > 0.0 && rho < (double)INFINITY;
                    if (seen) {
                        if (a.kind == PN_CAM_PANO) {
                            const double phi = atan2(hypot(v[0], v[2]), v[1]), theta = atan2(v[0], v[2]);
                            double t = -theta / (2.0 * kPiD);
                            t = t - floor(t);
                            qx = t * (double)a.Wm;
                            qy = phi / kPiD * (double)a.Hm;
                        } else {
                            seen = cube_pos<double>(a.Wm, v, qx, qy, face);
                        }
                    }
                    if (seen) {
                        double slope = 0.0;
                        if (a.normals) {
                            const double s2 = 1.0 - NoL * NoL;
                            double tn = sqrt(s2 > 0.0 ? s2 : 0.0) / NoL;
                            tn = tn < 10.0 ? tn : 10.0;
                            slope = ((((a.bias_slope * rho) * delta) * tn) * (double)(k + 1)) / 2.0;
                        }
                        const double scale = 1.0 + a.bias_rel;
                        const float* map = a.maps + (int64_t)li * a.Hm * a.Wm;
                        double sum = 0.0;
#pragma unroll 1
                        for (int b = 0; b < k; ++b) {
#pragma unroll 1
                            for (int c = 0; c < k; ++c) {
                                sum = sum + pcf_sample(map, a.kind, a.Hm, a.Wm, face, qx + (double)(c - half),
                                                       qy + (double)(b - half), rho, scale, a.bias_abs, slope);
                            }
                        }
                        V = sum / (double)(k * k);
                    }
                }
            }
        }
        if (a.visibility) a.visibility[r * a.L + li] = (float)V;
        if (V > 0.0) {
            const double rm = lt[11];
            const double den = r2 > rm * rm ? r2 : rm * rm;
#pragma unroll
            for (int q = 0; q < 3; ++q) E[q] = E[q] + (((double)lt[3 + q] * g) * V) / den;
        }
    }
    if (a.out || a.direct) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double dq = valid ? ((double)a.albedo[r * 3 + q] / kPiD) * E[q] : 0.0;
            if (a.direct) a.direct[r * 3 + q] = (float)dq;
            if (a.out) a.out[r * 3 + q] = (float)(a.ambient * (double)a.rgb[r * 3 + q] + dq);
        }
    }
}

}  // namespace

extern "C" {

int pn_relight(int64_t R, const float* origins, const float* directions, const float* depth, const float* normals,
               const float* albedo, const float* rgb, int L, const float* lights, int map_kind, int Hm, int Wm,
               const float* maps, float ambient, float normal_offset, float bias_abs, float bias_rel, float bias_slope,
               int pcf, float* out, float* direct, float* visibility, void* stream) {
    if (R < 0 || L < 0 || pcf < 1 || pcf > PN_RELIGHT_MAX_PCF || pcf % 2 == 0) return PN_ERR_BAD_SHAPE;
    if (!(isfinite(ambient) && isfinite(normal_offset) && isfinite(bias_abs) && isfinite(bias_rel) && isfinite(bias_slope)))
        return PN_ERR_BAD_SHAPE;
    if (bias_abs < 0.f || bias_rel < 0.f || bias_slope < 0.f) return PN_ERR_BAD_SHAPE;
    if (map_kind != PN_CAM_PANO && map_kind != PN_CAM_CUBE) return PN_ERR_UNSUPPORTED;
    if (Hm < 2 || Wm < 2 || (int64_t)Hm * Wm >= ((int64_t)1 << 31)) return PN_ERR_BAD_SHAPE;
    if (map_kind == PN_CAM_CUBE && (int64_t)Hm != 6 * (int64_t)Wm) return PN_ERR_BAD_SHAPE;
    if (R == 0) return PN_OK;
    if (!origins || !directions || !depth) return PN_ERR_NULL;
    if (L > 0 && (!lights || !maps)) return PN_ERR_NULL;
    if ((out || direct) && (!albedo || !rgb)) return PN_ERR_NULL;
    if (!out && !direct && !visibility) return PN_OK;
    RelightArgs a{R, origins, directions, depth, normals, albedo, rgb, L, lights, map_kind, Hm, Wm, maps,
                  (double)ambient, (double)normal_offset, (double)bias_abs, (double)bias_rel, (double)bias_slope, pcf,
                  out, direct, visibility};
    hipLaunchKernelGGL(k_relight, dim3(nblk(R, kThreads)), dim3(kThreads), 0, ST(stream), a);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
