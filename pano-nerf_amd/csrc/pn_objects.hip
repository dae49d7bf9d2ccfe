// pn_objects.hip — virtual object insertion (gfx950): the ray / triangle tracer and the differential-rendering shadow an
// inserted mesh casts on the scene, each one kernel template over pn_tri.h's two finders (brute force, and a walk of
// pn_bvh.hip's tree); the reference's surface shading (Lambertian and microfacet, utils/surface_rendering.py:6-61,
// 129-203) with a light probe's pixels as the lights, hit attributes and the composite.
// Conventions (edge rule, tie-break, direction of v, shadow definition) are stated in include/panonerf_hip.h.
//
// One ray / hit pixel / scene point per thread; what the threads of a workgroup share (triangles, probe pixels) goes
// through LDS in tiles.  The tracer's arithmetic is fp32 in a fixed order of separate operations (the library builds
// with -ffp-contract=off), the same function for primary and shadow rays.  Every sum is fp64 in pixel order, without
// atomics: two calls on the same inputs give the same bits, whatever the number of rows per launch.
#include "pn_common.h"
#include "pn_probes.h"
#include "pn_tri.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 256;  // probe pixels staged per LDS tile
constexpr int kMaxProbes = PN_OBJ_MAX_PROBES;

// row f of tris [F, 12]: v0, 0, e1 = v1 - v0, 0, e2 = v2 - v0, 0.  A face with an index outside [0, V) becomes the
// all-zero triangle, which no ray hits (det == 0).
__global__ __launch_bounds__(kThreads) void k_tri_setup(int64_t F, int64_t V, const float* vertices, const int32_t* faces,
                                                       float4* tris) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), e1 = v0, e2 = v0;
    if (a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V) {
        const float *pa = vertices + a * 3, *pb = vertices + b * 3, *pc = vertices + c * 3;
        v0 = make_float4(pa[0], pa[1], pa[2], 0.f);
        e1 = make_float4(pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2], 0.f);
        e2 = make_float4(pc[0] - pa[0], pc[1] - pa[1], pc[2] - pa[2], 0.f);
    }
    tris[f * 3] = v0;
    tris[f * 3 + 1] = e1;
    tris[f * 3 + 2] = e2;
}

using pn_tri::BruteFinder;
using pn_tri::BvhFinder;
using pn_tri::Hit;
using pn_tri::reaches_sphere;

// closest hit of ray r with the F triangles, as Finder finds it; any != 0: whether there is one.  bs may be NULL, and a
// finder that walks nodes is never given one (its root box does that job; pn_trace_mesh_bvh takes no sphere), so that
// instance compiles the test out.
template <class Finder>
__global__ __launch_bounds__(Finder::kThreads) void k_trace(int64_t R, const float* origins, const float* dirs, int64_t F,
                                                           const float4* tris, const float4* nodes, const float* t_max,
                                                           int any, const float* bs, float* t_out, int32_t* face_out,
                                                           float* bary_out, uint8_t* hit_out) {
    __shared__ typename Finder::Shared s_find;
    const int64_t r = (int64_t)blockIdx.x * Finder::kThreads + threadIdx.x;
    const bool live = r < R;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    Hit h{INFINITY, 0.f, 0.f, -1};
    if (live) {
        ox = origins[r * 3], oy = origins[r * 3 + 1], oz = origins[r * 3 + 2];
        dx = dirs[r * 3], dy = dirs[r * 3 + 1], dz = dirs[r * 3 + 2];
        if (t_max) h.best = t_max[r];
    }
    Finder finder(F, tris, nodes, s_find);
    const bool reach = Finder::kNodes || !bs || reaches_sphere(ox, oy, oz, dx, dy, dz, bs);
    finder.find(live && reach, ox, oy, oz, dx, dy, dz, any != 0, h);
    if (!live) return;
    if (any) {
        hit_out[r] = h.face >= 0;
        return;
    }
    t_out[r] = h.face >= 0 ? h.best : INFINITY;
    face_out[r] = h.face;
    bary_out[r * 2] = h.u;
    bary_out[r * 2 + 1] = h.v;
}

// reference shading of row r under the light sum_k w[r, k] L_k(pix) (fp64 throughout, pixels in order):
//   Lambert (mode 0): shading = sum L relu(n . l) omega, diffuse = albedo / pi shading, specular = 0
//   microfacet (mode 1): microfeast_brdf with v = -viewdir; diffuse = albedo / pi sum L NoL omega,
//                        specular = sum spec L omega, spec = D F G / (4 NoL NoV) with NaN and +inf -> 0
__global__ __launch_bounds__(kThreads) void k_shade(int64_t R, int K, int64_t HW, Probes pr, const float* dirs,
                                                   const float* omega, const float* albedo, const float* normals,
                                                   const float* viewdirs, const float* roughness, float roughness_all,
                                                   int mode, const float* weights, float* rgb, float* diffuse,
                                                   float* specular, float* shading) {
    __shared__ double4 s_dir[kTile];                // l, omega
    __shared__ float s_rad[kMaxProbes * kTile * 3];  // L_k(pix), channel-minor
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = r < R;
    double nx = 0.0, ny = 0.0, nz = 0.0, vx = 0.0, vy = 0.0, vz = 0.0, rough = 0.0;
    double w[kMaxProbes];
#pragma unroll
    for (int k = 0; k < kMaxProbes; ++k) w[k] = k == 0 ? 1.0 : 0.0;
    if (live) {
        nx = normals[r * 3], ny = normals[r * 3 + 1], nz = normals[r * 3 + 2];
        vx = -(double)viewdirs[r * 3], vy = -(double)viewdirs[r * 3 + 1], vz = -(double)viewdirs[r * 3 + 2];
        rough = roughness ? (double)roughness[r] : (double)roughness_all;
        if (weights) {
#pragma unroll
            for (int k = 0; k < kMaxProbes; ++k)
                if (k < K) w[k] = weights[r * K + k];
        }
    }
    double NoV = nx * vx + ny * vy + nz * vz;
    NoV = NoV < 0.0 ? 0.0 : NoV;
    const double alpha = rough * rough, kk = rough * rough / 2.0, a2 = alpha * alpha;
    const double g2 = NoV / ((1.0 - kk) * NoV + kk);
    double d0 = 0.0, d1 = 0.0, d2 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t base = 0; base < HW; base += kTile) {
        const int cnt = (int)((HW - base) < kTile ? (HW - base) : kTile);
        for (int t = threadIdx.x; t < cnt; t += kThreads) {
            const int64_t pix = base + t;
            s_dir[t] = make_double4(dirs[pix * 3], dirs[pix * 3 + 1], dirs[pix * 3 + 2], omega[pix]);
            for (int k = 0; k < K; ++k) {
                const float* xp = pr.x + k * pr.probe_stride + pix * pr.ps;
                float* o = s_rad + (k * kTile + t) * 3;
                o[0] = xp[0], o[1] = xp[pr.cs], o[2] = xp[2 * pr.cs];
            }
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const double4 l = s_dir[t];
            double L0 = 0.0, L1 = 0.0, L2 = 0.0;
#pragma unroll
            for (int k = 0; k < kMaxProbes; ++k) {
                if (k < K) {
                    const float* x = s_rad + (k * kTile + t) * 3;
                    L0 += w[k] * (double)x[0], L1 += w[k] * (double)x[1], L2 += w[k] * (double)x[2];
                }
            }
            L0 *= l.w, L1 *= l.w, L2 *= l.w;
            double NoL = nx * l.x + ny * l.y + nz * l.z;
            NoL = NoL < 0.0 ? 0.0 : NoL;  // relu as torch evaluates it: NaN stays NaN
            d0 += L0 * NoL, d1 += L1 * NoL, d2 += L2 * NoL;
            if (mode == 1 && !(NoL == 0.0)) {  // NoL == 0: G1 = 0 and the quotient is 0 / 0 -> NaN -> 0 upstream
                double hx = l.x + vx, hy = l.y + vy, hz = l.z + vz;
                double hn = sqrt(hx * hx + hy * hy + hz * hz);
                hn = hn < 1e-12 ? 1e-12 : hn;  // F.normalize
                hx /= hn, hy /= hn, hz /= hn;
                double NoH = nx * hx + ny * hy + nz * hz, VoH = vx * hx + vy * hy + vz * hz;
                NoH = NoH < 0.0 ? 0.0 : NoH;
                VoH = VoH < 0.0 ? 0.0 : VoH;
                const double den = (NoH * NoH) * (a2 - 1.0) + 1.0;
                const double D = a2 / (M_PI * (den * den));
                const double Fr = 0.04 + (1.0 - 0.04) * exp2(-(5.55473 * VoH + 6.98316) * VoH);
                const double g1 = NoL / ((1.0 - kk) * NoL + kk);
                double sp = D * Fr * (g1 * g2) / (4.0 * NoL * NoV);
                if (isnan(sp) || sp == (double)INFINITY) sp = 0.0;
                s0 += sp * L0, s1 += sp * L1, s2 += sp * L2;
            }
        }
        __syncthreads();
    }
    if (!live) return;
    const double e[3] = {d0, d1, d2}, s[3] = {s0, s1, s2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float df = (float)((double)albedo[r * 3 + c] / M_PI * e[c]);
        const float sf = mode == 1 ? (float)s[c] : 0.f;
        diffuse[r * 3 + c] = df;
        specular[r * 3 + c] = sf;
        rgb[r * 3 + c] = df + sf;
        if (shading) shading[r * 3 + c] = (float)e[c];
    }
}

// ratio[r] = E(unoccluded) / E(all), E(S) = sum_{pix in S} mean_c L(pix) relu(n . l_pix) omega_pix; pix is occluded when
// the ray from fl(x + fl(bias n)) along l_pix hits a triangle (t > 0), which is what Finder is asked.  One point per
// thread; the workgroup walks the probe's pixels together, in order.  Pixels below the point's horizon, pixels whose ray
// cannot reach the mesh's bounding sphere and points whose hemisphere cannot see it are never asked about.
template <class Finder>
__global__ __launch_bounds__(Finder::kThreads) void k_shadow(int64_t R, int64_t HW, Probes pr, const float* dirs,
                                                            const float* omega, const float* points,
                                                            const float* normals, float bias, int64_t F,
                                                            const float4* tris, const float4* nodes, const float* bs,
                                                            float* out) {
    __shared__ double4 s_dir[kTile];  // l, mean_c L omega
    __shared__ typename Finder::Shared s_find;
    const int64_t r = (int64_t)blockIdx.x * Finder::kThreads + threadIdx.x;
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
    Finder finder(F, tris, nodes, s_find);
    for (int64_t base = 0; base < HW; base += kTile) {
        const int cnt = (int)((HW - base) < kTile ? (HW - base) : kTile);
        for (int t = threadIdx.x; t < cnt; t += Finder::kThreads) {
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
            Hit h{INFINITY, 0.f, 0.f, -1};
            finder.find(sees && c > 0.0 && reaches_sphere(ox, oy, oz, l.x, l.y, l.z, bs), ox, oy, oz, (float)l.x,
                        (float)l.y, (float)l.z, true, h);  // (float) is exact: the table is fp32
            if (h.face < 0) e_un += wgt;
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

struct HitArgs {
    const float *origins, *dirs, *t, *bary, *scene_dep, *vertices, *vnormals, *valbedo, *probe_pos;
    const int32_t *face, *faces;
    int64_t F, V;
    float albedo[3];
    int K;
    uint8_t* mask;
    float *points, *normals, *albedo_out, *viewdirs, *weights, *scene_points;
};

// per ray: mask = hit and not (t >= scene depth); for a masked ray the hit point o + t d, the shading normal
// (barycentric blend of the vertex normals, or normalize(e1 x e2)), flipped towards the eye, the albedo, the unit
// camera-to-surface direction and the probe weights; zeros elsewhere.  scene_points = o + d scene_dep outside the mask,
// NaN inside (a NaN point's shadow ratio is 1).  Arithmetic in fp64 on the fp32 inputs, rounded once.
__global__ __launch_bounds__(kThreads) void k_object_hits(int64_t R, HitArgs a) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const int32_t f = a.face[r];
    const float t = a.t[r];
    const double ox = a.origins[r * 3], oy = a.origins[r * 3 + 1], oz = a.origins[r * 3 + 2];
    const double dx = a.dirs[r * 3], dy = a.dirs[r * 3 + 1], dz = a.dirs[r * 3 + 2];
    bool m = f >= 0 && f < a.F;
    int64_t i0 = 0, i1 = 0, i2 = 0;
    if (m) {
        i0 = a.faces[(int64_t)f * 3], i1 = a.faces[(int64_t)f * 3 + 1], i2 = a.faces[(int64_t)f * 3 + 2];
        m = i0 >= 0 && i0 < a.V && i1 >= 0 && i1 < a.V && i2 >= 0 && i2 < a.V;
    }
    if (m && a.scene_dep) m = !(t >= a.scene_dep[r]);
    a.mask[r] = m;
    float out[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) out[i] = 0.f;
    double hx = 0.0, hy = 0.0, hz = 0.0;
    if (m) {
        const double u = a.bary[r * 2], v = a.bary[r * 2 + 1], w0 = 1.0 - u - v;
        hx = ox + (double)t * dx, hy = oy + (double)t * dy, hz = oz + (double)t * dz;
        const double dn = sqrt(dx * dx + dy * dy + dz * dz);
        const double wx = dx / dn, wy = dy / dn, wz = dz / dn;
        double nx, ny, nz;
        if (a.vnormals) {
            const float *n0 = a.vnormals + i0 * 3, *n1 = a.vnormals + i1 * 3, *n2 = a.vnormals + i2 * 3;
            nx = w0 * n0[0] + u * n1[0] + v * n2[0];
            ny = w0 * n0[1] + u * n1[1] + v * n2[1];
            nz = w0 * n0[2] + u * n1[2] + v * n2[2];
        } else {
            const float *p0 = a.vertices + i0 * 3, *p1 = a.vertices + i1 * 3, *p2 = a.vertices + i2 * 3;
            const double ax = (double)p1[0] - p0[0], ay = (double)p1[1] - p0[1], az = (double)p1[2] - p0[2];
            const double bx = (double)p2[0] - p0[0], by = (double)p2[1] - p0[1], bz = (double)p2[2] - p0[2];
            nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        }
        double nn = sqrt(nx * nx + ny * ny + nz * nz);
        nn = nn < 1e-30 ? 1e-30 : nn;
        nx /= nn, ny /= nn, nz /= nn;
        if (nx * wx + ny * wy + nz * wz > 0.0) nx = -nx, ny = -ny, nz = -nz;  // n . v < 0 with v = -w
        out[0] = (float)hx, out[1] = (float)hy, out[2] = (float)hz;
        out[3] = (float)nx, out[4] = (float)ny, out[5] = (float)nz;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            out[6 + c] = a.valbedo ? (float)(w0 * a.valbedo[i0 * 3 + c] + u * a.valbedo[i1 * 3 + c] +
                                             v * a.valbedo[i2 * 3 + c])
                                   : a.albedo[c];
        }
        out[9] = (float)wx, out[10] = (float)wy, out[11] = (float)wz;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.points[r * 3 + c] = out[c];
        a.normals[r * 3 + c] = out[3 + c];
        a.albedo_out[r * 3 + c] = out[6 + c];
        a.viewdirs[r * 3 + c] = out[9 + c];
    }
    if (a.scene_points) {
        const double sd = a.scene_dep ? (double)a.scene_dep[r] : (double)NAN;
        a.scene_points[r * 3] = m ? NAN : (float)(ox + sd * dx);
        a.scene_points[r * 3 + 1] = m ? NAN : (float)(oy + sd * dy);
        a.scene_points[r * 3 + 2] = m ? NAN : (float)(oz + sd * dz);
    }
    if (a.weights) {
        // normalised inverse distances to the probe positions; a position within 1e-6 takes its probe alone (the first)
        double inv[kMaxProbes], sum = 0.0;
        int exact = -1;
#pragma unroll
        for (int k = 0; k < kMaxProbes; ++k) {
            inv[k] = 0.0;
            if (k < a.K && m) {
                const double ex = hx - a.probe_pos[k * 3], ey = hy - a.probe_pos[k * 3 + 1], ez = hz - a.probe_pos[k * 3 + 2];
                const double dist = sqrt(ex * ex + ey * ey + ez * ez);
                if (dist <= 1e-6) {
                    if (exact < 0) exact = k;
                } else {
                    inv[k] = 1.0 / dist;
                }
                sum += inv[k];
            }
        }
#pragma unroll
        for (int k = 0; k < kMaxProbes; ++k) {
            if (k < a.K) {
                float wk = 0.f;
                if (m) wk = exact >= 0 ? (k == exact ? 1.f : 0.f) : (float)(inv[k] / sum);
                a.weights[r * a.K + k] = wk;
            }
        }
    }
}

// rgb = mask ? object_rgb : scene_rgb * shadow (one fp32 product), depth = mask ? t : scene_dep
__global__ __launch_bounds__(kThreads) void k_object_composite(int64_t R, const uint8_t* mask, const float* object_rgb,
                                                              const float* t, const float* scene_rgb,
                                                              const float* scene_dep, const float* shadow, float* rgb,
                                                              float* depth) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    const bool m = mask[r] != 0;
    const float s = shadow[r];
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[r * 3 + c] = m ? object_rgb[r * 3 + c] : scene_rgb[r * 3 + c] * s;
    depth[r] = m ? t[r] : scene_dep[r];
}

bool rows_ok(int64_t n, int threads = kThreads) { return n >= 0 && n < ((int64_t)1 << 31) * threads / 2; }
bool probe_ok(int H, int W) { return H >= 2 && W >= 2 && (int64_t)H * W < ((int64_t)1 << 30); }

// the checks and the launch behind pn_trace_mesh and pn_trace_mesh_bvh (nodes: only a finder that walks them wants them)
template <class Finder>
int trace_mesh(int64_t R, const float* origins, const float* directions, int64_t F, const float* tris, const float* nodes,
               const float* t_max, const float* bsphere, int any_hit, float* t, int32_t* face, float* bary, uint8_t* hit,
               void* stream) {
    if (!rows_ok(R, Finder::kThreads) || F <= 0 || F >= ((int64_t)1 << 31)) return PN_ERR_BAD_SHAPE;
    if (R == 0) return PN_OK;
    if (!origins || !directions || !tris || (Finder::kNodes && !nodes)) return PN_ERR_NULL;
    if (any_hit ? !hit : (!t || !face || !bary)) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_trace<Finder>, dim3(nblk(R, Finder::kThreads)), dim3(Finder::kThreads), 0, ST(stream), R, origins,
                       directions, F, (const float4*)tris, (const float4*)nodes, t_max, any_hit, bsphere, t, face, bary,
                       hit);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

// the same for pn_shadow_ratio and pn_shadow_ratio_bvh
template <class Finder>
int shadow_ratio(int64_t R, int H, int W, const float* x, int64_t cs, int64_t ps, const float* dirs, const float* omega,
                 const float* points, const float* normals, float bias, int64_t F, const float* tris, const float* nodes,
                 const float* bsphere, float* out, void* stream) {
    if (!rows_ok(R, Finder::kThreads) || F < 0 || F >= ((int64_t)1 << 31) || !probe_ok(H, W)) return PN_ERR_BAD_SHAPE;
    if (R == 0) return PN_OK;
    if (!x || !dirs || !omega || !points || !normals || !out) return PN_ERR_NULL;
    if (F > 0 && (!tris || !bsphere || (Finder::kNodes && !nodes))) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_shadow<Finder>, dim3(nblk(R, Finder::kThreads)), dim3(Finder::kThreads), 0, ST(stream), R,
                       (int64_t)H * W, Probes{x, 0, cs, ps}, dirs, omega, points, normals, bias, F, (const float4*)tris,
                       (const float4*)nodes, bsphere, out);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_tri_setup(int64_t F, int64_t V, const float* vertices, const int32_t* faces, float* tris, void* stream) {
    if (F < 0 || V < 0 || F >= ((int64_t)1 << 31)) return PN_ERR_BAD_SHAPE;
    if (F == 0) return PN_OK;
    if (!vertices || !faces || !tris) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_tri_setup, dim3(nblk(F, kThreads)), dim3(kThreads), 0, ST(stream), F, V, vertices, faces,
                       (float4*)tris);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_trace_mesh(int64_t R, const float* origins, const float* directions, int64_t F, const float* tris,
                  const float* t_max, const float* bsphere, int any_hit, float* t, int32_t* face, float* bary,
                  uint8_t* hit, void* stream) {
    return trace_mesh<BruteFinder>(R, origins, directions, F, tris, nullptr, t_max, bsphere, any_hit, t, face, bary, hit,
                                   stream);
}

int pn_trace_mesh_bvh(int64_t R, const float* origins, const float* directions, int64_t F, const float* tris,
                      const float* nodes, const float* t_max, int any_hit, float* t, int32_t* face, float* bary,
                      uint8_t* hit, void* stream) {
    return trace_mesh<BvhFinder>(R, origins, directions, F, tris, nodes, t_max, nullptr, any_hit, t, face, bary, hit,
                                 stream);
}

int pn_shade(int64_t R, int K, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps,
             const float* dirs, const float* omega, const float* albedo, const float* normals, const float* viewdirs,
             const float* roughness, float roughness_all, int microfacet, const float* weights, float* rgb,
             float* diffuse, float* specular, float* shading, void* stream) {
    if (!rows_ok(R) || K < 1 || K > kMaxProbes || !probe_ok(H, W)) return PN_ERR_BAD_SHAPE;
    if (R == 0) return PN_OK;
    if (!x || !dirs || !omega || !albedo || !normals || !viewdirs || !rgb || !diffuse || !specular) return PN_ERR_NULL;
    if (K > 1 && !weights) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_shade, dim3(nblk(R, kThreads)), dim3(kThreads), 0, ST(stream), R, K, (int64_t)H * W,
                       Probes{x, probe_stride, cs, ps}, dirs, omega, albedo, normals, viewdirs, roughness,
                       roughness_all, microfacet ? 1 : 0, weights, rgb, diffuse, specular, shading);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_shadow_ratio(int64_t R, int H, int W, const float* x, int64_t cs, int64_t ps, const float* dirs,
                    const float* omega, const float* points, const float* normals, float bias, int64_t F,
                    const float* tris, const float* bsphere, float* out, void* stream) {
    return shadow_ratio<BruteFinder>(R, H, W, x, cs, ps, dirs, omega, points, normals, bias, F, tris, nullptr, bsphere,
                                     out, stream);
}

int pn_shadow_ratio_bvh(int64_t R, int H, int W, const float* x, int64_t cs, int64_t ps, const float* dirs,
                        const float* omega, const float* points, const float* normals, float bias, int64_t F,
                        const float* tris, const float* nodes, const float* bsphere, float* out, void* stream) {
    return shadow_ratio<BvhFinder>(R, H, W, x, cs, ps, dirs, omega, points, normals, bias, F, tris, nodes, bsphere, out,
                                   stream);
}

int pn_object_hits(int64_t R, const float* origins, const float* directions, const float* t, const int32_t* face,
                   const float* bary, const float* scene_dep, int64_t V, const float* vertices, int64_t F,
                   const int32_t* faces, const float* vertex_normals, const float* vertex_albedo, float albedo_r,
                   float albedo_g, float albedo_b, int K, const float* probe_positions, uint8_t* mask, float* points,
                   float* normals, float* albedo, float* viewdirs, float* weights, float* scene_points, void* stream) {
    if (!rows_ok(R) || V < 0 || F < 0 || K < 1 || K > kMaxProbes) return PN_ERR_BAD_SHAPE;
    if (R == 0) return PN_OK;
    if (!origins || !directions || !t || !face || !bary || !mask || !points || !normals || !albedo || !viewdirs)
        return PN_ERR_NULL;
    if (F > 0 && (!vertices || !faces)) return PN_ERR_NULL;
    if (weights && !probe_positions) return PN_ERR_NULL;
    if (scene_points && !scene_dep) return PN_ERR_NULL;
    HitArgs a{origins, directions, t, bary, scene_dep, vertices, vertex_normals, vertex_albedo, probe_positions,
              face, faces, F, V, {albedo_r, albedo_g, albedo_b}, K, mask, points, normals, albedo, viewdirs,
              weights, scene_points};
    hipLaunchKernelGGL(k_object_hits, dim3(nblk(R, kThreads)), dim3(kThreads), 0, ST(stream), R, a);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_object_composite(int64_t R, const uint8_t* mask, const float* object_rgb, const float* t,
                        const float* scene_rgb, const float* scene_dep, const float* shadow, float* rgb, float* depth,
                        void* stream) {
    if (!rows_ok(R)) return PN_ERR_BAD_SHAPE;
    if (R == 0) return PN_OK;
    if (!mask || !object_rgb || !t || !scene_rgb || !scene_dep || !shadow || !rgb || !depth) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_object_composite, dim3(nblk(R, kThreads)), dim3(kThreads), 0, ST(stream), R, mask, object_rgb,
                       t, scene_rgb, scene_dep, shadow, rgb, depth);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
