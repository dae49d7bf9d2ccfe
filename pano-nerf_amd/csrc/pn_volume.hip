// pn_volume.hip — the baked radiance volume (gfx950): brick occupancy of a packed [nx, ny, nz, C] volume and the ray
// marcher that renders it with no network in the loop.  The contract (lattice, trilinear tap, SH colour, compositing, depth
// rule, what a jump may skip) is stated term for term in include/panonerf_hip.h, section "radiance volume", and restated
// in numpy by tests/_volume_ref.py.
//
// k_volume_march: one ray per thread, 64 threads (one wave) per workgroup.  Rows arrive in pixel order, so the lanes of a
// wave march neighbouring rays through the same bricks and their 8-corner taps fall on the same cache lines (a corner is
// one contiguous run of C floats); a wave per ray would need a scan over the transmittance and leave 63 lanes idle on
// the short rays that dominate after early termination.  One wave per workgroup keeps a long ray from holding three
// other waves' slots.  Everything a ray carries lives in registers (every array is indexed by unrolled loops only): no LDS,
// no scratch, no atomics; fp64 on the fp32 inputs, each output rounded once, so two calls give the same bits.
//
// Jumps never rest on an epsilon.  Every grid coordinate is a chain of correctly rounded + - * / on (k + 0.5), and rounding
// is monotone, so the computed coordinate of axis a is a monotone function of the lattice index k.  A jump proposes its last
// skipped point kl from the exit plane and then EVALUATES point kl with the sampling formula itself: if k and kl are both in
// the brick (or both beyond the same box face), so is every point between them.  A proposal that fails falls back to kl - 1,
// then to no jump at all.
#include "pn_common.h"

namespace {

constexpr int kThreads = 64;
constexpr int kBrick = PN_VOLUME_BRICK;
constexpr int kShift = 3;  // log2(kBrick)
static_assert(kBrick == 1 << kShift, "brick size");

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// ---------------------------------------------------------------------------------------------------------- occupancy
// one wave per brick: the lanes stride over the brick's (up to 9^3) vertices; a brick is occupied iff one has sigma > 0
__global__ __launch_bounds__(kThreads) void k_volume_occupancy(int nx, int ny, int nz, int C, const float* __restrict__ data,
                                                               int nby, int nbz, uint8_t* __restrict__ occ) {
    const int64_t brick = blockIdx.x;
    const int bk = (int)(brick % nbz), bj = (int)((brick / nbz) % nby), bi = (int)(brick / ((int64_t)nbz * nby));
    const int i0 = bi * kBrick, j0 = bj * kBrick, k0 = bk * kBrick;
    const int ni = imin(i0 + kBrick, nx - 1) - i0 + 1, nj = imin(j0 + kBrick, ny - 1) - j0 + 1,
              nk = imin(k0 + kBrick, nz - 1) - k0 + 1;
    const int total = ni * nj * nk;
    bool any = false;
    for (int t = threadIdx.x; t < total; t += kThreads) {
        const int dk = t % nk, dj = (t / nk) % nj, di = t / (nk * nj);  // i0 + di <= nx - 1 and so on: inside the tensor
        const int64_t v = ((int64_t)(i0 + di) * ny + (j0 + dj)) * nz + (k0 + dk);
        any = any || data[v * C] > 0.f;  // a NaN is not > 0
    }
    const bool hit = __ballot(any) != 0;
    if (threadIdx.x == 0) occ[brick] = hit ? 1 : 0;
}

// -------------------------------------------------------------------------------------------------------------- march
struct MarchArgs {
    int64_t R;
    int n[3];  // vertices per axis
    int E;     // attribute channels
    const float* data;
    const uint8_t* occ;  // null: no brick jumps
    double lo[3], st[3];
    const float *origins, *directions, *near, *far;
    double step, t_min;
    float *rgb, *depth, *acc, *attrs;
    int32_t* taps;  // [R, 2]: trilinear taps taken for sigma, and of those the ones that went on to the colour
};

__device__ __forceinline__ bool finite_d(double x) { return x - x == 0.0; }

// the last point to skip, from the lattice position s of an exit plane: floor(s) held to [k, n - 1]; a NaN proposes k
__device__ __forceinline__ int propose(double s, int k, int n) {
    if (!(s > (double)k)) return k;
    if (s >= (double)(n - 1)) return n - 1;
    return (int)floor(s);
}

template <int kDeg, int kEmax>
__global__ __launch_bounds__(kThreads) void k_volume_march(MarchArgs a) {
    constexpr int K = (kDeg + 1) * (kDeg + 1);
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= a.R) return;
    const int C = 1 + 3 * K + a.E;
    double o[3], d[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        o[x] = (double)a.origins[3 * r + x];
        d[x] = (double)a.directions[3 * r + x];
    }
    const double tn = (double)a.near[r], tf = (double)a.far[r];
    bool valid = finite_d(tn) && finite_d(tf);
#pragma unroll
    for (int x = 0; x < 3; ++x) valid = valid && finite_d(o[x]) && finite_d(d[x]);
    const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    valid = valid && len > 0.0 && tf > tn;
    double dt = 0.0, nd = 0.0;
    if (valid) {
        dt = a.step / len;
        nd = ceil((tf - tn) / dt);
        valid = nd < 2147483648.0;  // an infinite or NaN count fails too
    }
    double rgb[3] = {0.0, 0.0, 0.0}, at[kEmax > 0 ? kEmax : 1], acc = 0.0, wt = 0.0;
#pragma unroll
    for (int e = 0; e < kEmax; ++e) at[e] = 0.0;
    float depth = 0.f;
    int n_sigma = 0, n_colour = 0;
    if (valid) {
        const int n = (int)nd;
        const double stepw = dt * len;
        double Y[K];
        {
            const double x = d[0] / len, y = d[1] / len, z = d[2] / len;
            Y[0] = PN_SH_C0;
            if (kDeg >= 1) {
                Y[1] = PN_SH_C1 * y;
                Y[2] = PN_SH_C1 * z;
                Y[3] = PN_SH_C1 * x;
            }
            if (kDeg >= 2) {
                Y[4] = PN_SH_C2 * (x * y);
                Y[5] = PN_SH_C2 * (y * z);
                Y[6] = PN_SH_C3 * (3.0 * (z * z) - 1.0);
                Y[7] = PN_SH_C2 * (x * z);
                Y[8] = PN_SH_C4 * (x * x - y * y);
            }
        }
        // the grid coordinate of axis x at lattice point kk: THE sampling formula, also what every jump is checked with
        auto coord = [&](int x, int kk) -> double {
            const double t = tn + ((double)kk + 0.5) * dt;
            return ((o[x] + t * d[x]) - a.lo[x]) / a.st[x];
        };
        // the lattice position of the plane g_x = p: (t_plane - near) / dt - 0.5 (callers have d[x] != 0)
        auto plane = [&](int x, double p) -> double {
            return ((((a.lo[x] + p * a.st[x]) - o[x]) / d[x]) - tn) / dt - 0.5;
        };
        double T = 1.0;
        int k = 0;
        while (k < n) {
            const double t = tn + ((double)k + 0.5) * dt;
            double g[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) g[x] = ((o[x] + t * d[x]) - a.lo[x]) / a.st[x];
            // ---- outside the box: nothing to add; jump to the face ahead, or stop if the ray only moves away
            bool outside = false, gone = false;
            int kl = k;
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double top = (double)(a.n[x] - 1);
                const bool low = !(g[x] >= 0.0), high = g[x] > top;
                if (low || high) {
                    outside = true;
                    if (low ? !(d[x] > 0.0) : !(d[x] < 0.0)) {
                        gone = true;  // monotone coordinates: no later point comes back
                    } else {
                        int c = propose(plane(x, low ? 0.0 : top), k, n);
#pragma unroll 1
                        for (int tries = 0; tries < 2 && c > k; ++tries) {
                            const double gc = coord(x, c);
                            if (low ? !(gc >= 0.0) : gc > top) break;
                            c = tries == 0 ? c - 1 : k;
                        }
                        kl = c > kl ? c : kl;
                    }
                }
            }
            if (gone) break;
            if (outside) {
                k = kl + 1;
                continue;
            }
            // ---- the cell: g in [0, n - 1] on every axis, so 0 <= c <= n - 2 and every corner c, c + 1 is a vertex
            int c[3];
            double f[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double fl = floor(g[x]);
                c[x] = imin((int)fl, a.n[x] - 2);
                f[x] = g[x] - (double)c[x];
            }
            if (a.occ) {
                const int b0 = c[0] >> kShift, b1 = c[1] >> kShift, b2 = c[2] >> kShift;
                const int nb1 = (a.n[1] + kBrick - 2) >> kShift, nb2 = (a.n[2] + kBrick - 2) >> kShift;
                if (a.occ[((int64_t)b0 * nb1 + b1) * nb2 + b2] == 0) {
                    // every cell of this brick has corners <= 0 or NaN only: skip to the last lattice point still in it
                    const int b[3] = {b0, b1, b2};
                    double s = (double)(n - 1);
#pragma unroll
                    for (int x = 0; x < 3; ++x) {
                        if (d[x] != 0.0) {  // an axis the ray does not move along never leaves the brick: no division
                            const int up = imin((b[x] + 1) * kBrick, a.n[x] - 1);
                            const double sx = plane(x, d[x] > 0.0 ? (double)up : (double)(b[x] * kBrick));
                            s = sx < s ? sx : s;
                        }
                    }
                    int cand = propose(s, k, n);
#pragma unroll 1
                    for (int tries = 0; tries < 2 && cand > k; ++tries) {
                        bool same = true;
#pragma unroll
                        for (int x = 0; x < 3; ++x) {
                            const double gc = coord(x, cand);
                            const bool in = gc >= 0.0 && gc <= (double)(a.n[x] - 1);
                            const int cc = in ? imin((int)floor(gc), a.n[x] - 2) : -kBrick;
                            same = same && (cc >> kShift) == b[x];
                        }
                        if (same) break;
                        cand = tries == 0 ? cand - 1 : k;
                    }
                    k = cand + 1;
                    continue;
                }
            }
            // ---- the trilinear tap: weights (wx wy) wz, corners in the order i, j, k, low corner first
            double w[8];
            int64_t off[8];
            {
                const int64_t base = ((int64_t)c[0] * a.n[1] + c[1]) * a.n[2] + c[2];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int qi = q >> 2, qj = (q >> 1) & 1, qk = q & 1;
                    w[q] = ((qi ? f[0] : 1.0 - f[0]) * (qj ? f[1] : 1.0 - f[1])) * (qk ? f[2] : 1.0 - f[2]);
                    off[q] = (base + ((int64_t)qi * a.n[1] + qj) * a.n[2] + qk) * C;
                }
            }
            ++n_sigma;
            double sigma = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) sigma = sigma + w[q] * (double)a.data[off[q]];
            if (!(sigma > 0.0)) {
                ++k;
                continue;
            }
            ++n_colour;
            double col[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < K; ++kk) {
                double tri[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float* p = a.data + off[q] + 1 + 3 * kk;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) tri[ch] = tri[ch] + w[q] * (double)p[ch];
                }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) col[ch] = col[ch] + Y[kk] * tri[ch];
            }
            const double alpha = 1.0 - exp(-sigma * stepw);
            const double wgt = T * alpha;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) rgb[ch] = rgb[ch] + wgt * (col[ch] > 0.0 ? col[ch] : 0.0);
#pragma unroll
            for (int e = 0; e < kEmax; ++e) {
                if (e < a.E) {
                    double tri = 0.0;
#pragma unroll
                    for (int q = 0; q < 8; ++q) tri = tri + w[q] * (double)a.data[off[q] + 1 + 3 * K + e];
                    at[e] = at[e] + wgt * tri;
                }
            }
            acc = acc + wgt;
            wt = wt + wgt * t;
            T = T * (1.0 - alpha);
            if (T < a.t_min) break;
            ++k;
        }
        double q = wt / acc;
        if (q != q) q = 0.0;
        q = q > tn ? q : tn;
        q = q < tf ? q : tf;
        depth = (float)q;
    }
    if (a.rgb) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a.rgb[3 * r + ch] = (float)rgb[ch];
    }
    if (a.depth) a.depth[r] = depth;
    if (a.acc) a.acc[r] = (float)acc;
    if (a.taps) a.taps[2 * r] = n_sigma, a.taps[2 * r + 1] = n_colour;
    if (kEmax > 0 && a.attrs) {
#pragma unroll
        for (int e = 0; e < kEmax; ++e)
            if (e < a.E) a.attrs[(int64_t)a.E * r + e] = (float)at[e];
    }
}

bool grid_ok(int nx, int ny, int nz) {
    return nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz < ((int64_t)1 << 31);
}

template <int kDeg>
void launch_march(const MarchArgs& a, bool attrs, hipStream_t s) {
    const dim3 grid(nblk(a.R, kThreads)), block(kThreads);
    if (attrs)
        hipLaunchKernelGGL((k_volume_march<kDeg, PN_VOLUME_MAX_ATTR>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((k_volume_march<kDeg, 0>), grid, block, 0, s, a);
}

}  // namespace

extern "C" {

int64_t pn_volume_bricks(int nx, int ny, int nz) {
    if (!grid_ok(nx, ny, nz)) return -1;
    return (int64_t)((nx + kBrick - 2) >> kShift) * ((ny + kBrick - 2) >> kShift) * ((nz + kBrick - 2) >> kShift);
}

int pn_volume_occupancy(int nx, int ny, int nz, int channels, const float* data, uint8_t* occupancy, void* stream) {
    if (!grid_ok(nx, ny, nz) || channels < 1) return PN_ERR_BAD_SHAPE;
    if (!data || !occupancy) return PN_ERR_NULL;
    const int nby = (ny + kBrick - 2) >> kShift, nbz = (nz + kBrick - 2) >> kShift;
    const dim3 grid((unsigned)pn_volume_bricks(nx, ny, nz)), block(kThreads);
    hipLaunchKernelGGL(k_volume_occupancy, grid, block, 0, ST(stream), nx, ny, nz, channels, data, nby, nbz, occupancy);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_volume_march(int64_t R, int nx, int ny, int nz, int sh_degree, int E, const float* data, const uint8_t* occupancy,
                    float x0, float y0, float z0, float dx, float dy, float dz, const float* origins,
                    const float* directions, const float* near, const float* far, float step, float t_min, float* rgb,
                    float* depth, float* acc, float* attrs, int32_t* taps, void* stream) {
    const float lo[3] = {x0, y0, z0}, st[3] = {dx, dy, dz};
    bool ok = R >= 0 && R < ((int64_t)1 << 31) * kThreads && grid_ok(nx, ny, nz) && sh_degree >= 0 && sh_degree <= 2 &&
              E >= 0 && E <= PN_VOLUME_MAX_ATTR && step > 0.f && step < INFINITY && t_min >= 0.f && t_min < INFINITY;
    for (int x = 0; x < 3; ++x) ok = ok && lo[x] - lo[x] == 0.f && st[x] > 0.f && st[x] < INFINITY;
    if (!ok) return PN_ERR_BAD_SHAPE;
    if (R == 0) return PN_OK;
    if (!data || !origins || !directions || !near || !far) return PN_ERR_NULL;
    MarchArgs a{R, {nx, ny, nz}, E, data, occupancy, {}, {}, origins, directions, near, far, (double)step, (double)t_min,
                rgb, depth, acc, attrs, taps};
    for (int x = 0; x < 3; ++x) a.lo[x] = (double)lo[x], a.st[x] = (double)st[x];
    const bool with_attrs = E > 0 && attrs;
    switch (sh_degree) {
        case 0: launch_march<0>(a, with_attrs, ST(stream)); break;
        case 1: launch_march<1>(a, with_attrs, ST(stream)); break;
        default: launch_march<2>(a, with_attrs, ST(stream)); break;
    }
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
