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
//
// The marching loop exists once, as a template over a storage policy: the dense fp32 tensor with its occupancy bytes, or the
// brick pool (fp32 or fp16) behind its table, section "sparse radiance volume" of the header.  A policy answers two
// questions, "is this cell's brick present" and "corner q, channel ch, as fp64", and carries nothing across samples.
// k_volume_pack / k_volume_unpack move a volume between the two layouts.
//
// k_volume_march_bwd is the reverse of the compositing sweep for the dense store (header, "radiance volume: gradients"): it
// scatters dL/d(sigma, coefficients) as 64-bit integers, so that the sums are the same bits whatever the order;
// k_volume_grad_finish turns them into the fp32 gradient.
#include "pn_common.h"
#include "pn_probes.h"  // sh_basis

namespace {

constexpr int kThreads = 64;
constexpr int kBrick = PN_VOLUME_BRICK;
constexpr int kShift = 3;  // log2(kBrick)
static_assert(kBrick == 1 << kShift, "brick size");

constexpr int kEdge = kBrick + 1;                  // vertices along a brick's edge, the shared far face included
constexpr int kBrickVerts = kEdge * kEdge * kEdge;  // 729
constexpr int kCopyThreads = 256;                   // pack and unpack

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// bricks along an axis of n vertices (n - 1 cells), and the index of the brick of cell c in the [nbx, nby, nbz] tables
__host__ __device__ __forceinline__ int bricks_along(int n) { return (n + kBrick - 2) >> kShift; }
__device__ __forceinline__ int64_t brick_of(const int (&c)[3], const int (&n)[3]) {
    return ((int64_t)(c[0] >> kShift) * bricks_along(n[1]) + (c[1] >> kShift)) * bricks_along(n[2]) + (c[2] >> kShift);
}

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

// ------------------------------------------------------------------------------------------------------ pack / unpack
// one workgroup per brick (an absent one leaves at once); the lanes stride over the brick's 729 C values: contiguous stores
template <typename T>
__global__ __launch_bounds__(kCopyThreads) void k_volume_pack(int nx, int ny, int nz, int C, const int32_t* __restrict__ table,
                                                              int64_t B, const float* __restrict__ data,
                                                              const float* __restrict__ rows, int64_t M,
                                                              const int32_t* __restrict__ vertex_row, int nby, int nbz,
                                                              T* __restrict__ pool) {
    const int64_t brick = blockIdx.x;
    const int64_t slot = table[brick];
    if (slot < 0 || slot >= B) return;
    const int bk = (int)(brick % nbz), bj = (int)((brick / nbz) % nby), bi = (int)(brick / ((int64_t)nbz * nby));
    const int total = kBrickVerts * C;
    T* out = pool + slot * total;
    for (int t = threadIdx.x; t < total; t += kCopyThreads) {
        const int lv = t / C, ch = t - lv * C;
        const int i = bi * kBrick + lv / (kEdge * kEdge), j = bj * kBrick + (lv / kEdge) % kEdge, k = bk * kBrick + lv % kEdge;
        float v = 0.f;  // a local vertex past the grid's last vertex
        if (i < nx && j < ny && k < nz) {
            const int64_t vtx = ((int64_t)i * ny + j) * nz + k;
            if (data) {
                v = data[vtx * C + ch];
            } else {
                const int64_t row = vertex_row[vtx];
                if (row >= 0 && row < M) v = rows[row * C + ch];
            }
        }
        out[t] = (T)v;  // fp16: round to nearest even
    }
}

// one thread per dense vertex: read from the present brick of lowest index that holds it, 0 if none does
template <typename T>
__global__ __launch_bounds__(kCopyThreads) void k_volume_unpack(int nx, int ny, int nz, int C, const int32_t* __restrict__ table,
                                                                int64_t B, const T* __restrict__ pool, int nbx, int nby,
                                                                int nbz, float* __restrict__ data) {
    const int64_t v = (int64_t)blockIdx.x * kCopyThreads + threadIdx.x;
    if (v >= (int64_t)nx * ny * nz) return;
    const int g[3] = {(int)(v / ((int64_t)nz * ny)), (int)((v / nz) % ny), (int)(v % nz)};
    const int nb[3] = {nbx, nby, nbz};
    // per axis the lower candidate (brick b - 1, local 8: a shared face) and the upper one (brick b, local g & 7)
    int cb[3][2], cl[3][2];
    bool ok[3][2];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const int b = g[x] >> kShift, l = g[x] & (kBrick - 1);
        cb[x][0] = b - 1, cl[x][0] = kBrick, ok[x][0] = l == 0 && b >= 1;
        cb[x][1] = b, cl[x][1] = l, ok[x][1] = b < nb[x];
    }
    int64_t src = -1;
#pragma unroll
    for (int s = 0; s < 8; ++s) {  // ascending brick index: x slowest
        const int si = s >> 2, sj = (s >> 1) & 1, sk = s & 1;
        if (src < 0 && ok[0][si] && ok[1][sj] && ok[2][sk]) {
            const int64_t slot = table[((int64_t)cb[0][si] * nby + cb[1][sj]) * nbz + cb[2][sk]];
            if (slot >= 0 && slot < B)
                src = (slot * kBrickVerts + (cl[0][si] * kEdge + cl[1][sj]) * kEdge + cl[2][sk]) * C;
        }
    }
    for (int ch = 0; ch < C; ++ch) data[v * C + ch] = src >= 0 ? (float)pool[src + ch] : 0.f;
}

// -------------------------------------------------------------------------------------------------------------- march
// Storage policies.  present() says whether the cell's brick can hold a positive sigma, locate() prepares the tap of a
// cell in a present brick, value() is corner q (order i, j, k, low first), channel ch.  Tap is all a policy keeps, and only
// from present() to the end of the sample.
struct DenseStore {
    static constexpr bool kBricks = false;
    const float* data;
    const uint8_t* occ;  // null: no brick jumps
    struct Tap {
        int64_t off[8];
    };
    __device__ __forceinline__ bool jumps() const { return occ != nullptr; }
    __device__ __forceinline__ bool present(const int (&c)[3], const int (&n)[3], Tap&) const {
        return !occ || occ[brick_of(c, n)] != 0;
    }
    __device__ __forceinline__ void locate(const int (&c)[3], const int (&n)[3], int C, Tap& tap) const {
        const int64_t base = ((int64_t)c[0] * n[1] + c[1]) * n[2] + c[2];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            tap.off[q] = (base + ((int64_t)(q >> 2) * n[1] + ((q >> 1) & 1)) * n[2] + (q & 1)) * C;
    }
    __device__ __forceinline__ double value(const Tap& tap, int q, int ch) const { return (double)data[tap.off[q] + ch]; }
};

template <typename T>
struct BrickStore {
    static constexpr bool kBricks = true;
    const int32_t* table;
    const T* pool;
    int skip;
    struct Tap {
        int64_t base;  // the slot from present(), the value index of the low corner from locate()
        int C;
    };
    __device__ __forceinline__ bool jumps() const { return skip != 0; }
    __device__ __forceinline__ bool present(const int (&c)[3], const int (&n)[3], Tap& tap) const {
        tap.base = table[brick_of(c, n)];
        return tap.base >= 0;
    }
    __device__ __forceinline__ void locate(const int (&c)[3], const int (&)[3], int C, Tap& tap) const {
        constexpr int m = kBrick - 1;
        tap.base = (tap.base * kBrickVerts + ((c[0] & m) * kEdge + (c[1] & m)) * kEdge + (c[2] & m)) * C;
        tap.C = C;
    }
    __device__ __forceinline__ double value(const Tap& tap, int q, int ch) const {
        const int corner = ((q >> 2) * kEdge + ((q >> 1) & 1)) * kEdge + (q & 1);  // a constant once unrolled
        return (double)(float)pool[tap.base + (int64_t)corner * tap.C + ch];
    }
};

__device__ __forceinline__ bool finite_d(double x) { return x - x == 0.0; }

// the last point to skip, from the lattice position s of an exit plane: floor(s) held to [k, n - 1]; a NaN proposes k
__device__ __forceinline__ int propose(double s, int k, int n) {
    if (!(s > (double)k)) return k;
    if (s >= (double)(n - 1)) return n - 1;
    return (int)floor(s);
}

// what the marching loop reads: the volume, the rays and the two march parameters
template <class Store>
struct MarchRows {
    int64_t R;
    int n[3];  // vertices per axis
    int E;     // attribute channels
    Store store;
    double lo[3], st[3];
    const float *origins, *directions, *near, *far;
    double step, t_min;
};

// what the forward writes; a null output is not asked for
struct MarchOut {
    float *rgb, *depth, *acc, *attrs;
    int32_t* taps;  // [R, 2]: trilinear taps taken for sigma, and of those the ones that went on to the colour
};

// the reverse sweep's extra arguments (header, "radiance volume: gradients")
struct GradArgs {
    const float *g_rgb, *g_acc;  // [R, 3], [R]; null counts as zeros
    double inv_quantum;          // 1 / quantum: a power of two, so x * inv_quantum is x / quantum exactly
    long long* sums;             // [N, 1 + 3 K]
    int32_t* flag;
};

// one row's lattice (header, "Lattice"); valid false: the row marches nothing
struct Row {
    double o[3], d[3], tn, tf, len, dt;
    int n;
    bool valid;
};

template <class Store>
__device__ __forceinline__ Row load_row(const MarchRows<Store>& a, int64_t r) {
    Row row;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        row.o[x] = (double)a.origins[3 * r + x];
        row.d[x] = (double)a.directions[3 * r + x];
    }
    row.tn = (double)a.near[r], row.tf = (double)a.far[r];
    bool valid = finite_d(row.tn) && finite_d(row.tf);
#pragma unroll
    for (int x = 0; x < 3; ++x) valid = valid && finite_d(row.o[x]) && finite_d(row.d[x]);
    row.len = sqrt((row.d[0] * row.d[0] + row.d[1] * row.d[1]) + row.d[2] * row.d[2]);
    valid = valid && row.len > 0.0 && row.tf > row.tn;
    double nd = 0.0;
    row.dt = 0.0;
    if (valid) {
        row.dt = a.step / row.len;
        nd = ceil((row.tf - row.tn) / row.dt);
        valid = nd < 2147483648.0;  // an infinite or NaN count fails too
    }
    row.n = valid ? (int)nd : 0;
    row.valid = valid;
    return row;
}

// The lattice loop of every marcher, forward and reverse, over a valid row: gates, jumps, early stop.  on_tap() is called
// for every sigma tap (an absent brick without jumps, and each interpolated sigma); every sample that composites
// (sigma > 0) is handed to on_sample(c, w, tap, t, s, alpha, wgt, T): the cell, the corner weights, the located tap, the
// sample's t, the unclamped colour sums s_c, and T before the sample.
// Registers: inlined into k_volume_march the loop takes the dense degree-0 instance with attributes from 167 to 169 VGPRs,
// past the 168 of three waves per SIMD.  The forward's degree-0 instances hold the step by not carrying `far` through the
// loop: they read it again for the depth clamp.  profiles/volume_refactor.txt has every instance's registers and timings.
template <int kDeg, class Store, class FT, class FS>
__device__ __forceinline__ void march_row(const MarchRows<Store>& a, const Row& row,
                                          const double (&Y)[(kDeg + 1) * (kDeg + 1)], FT&& on_tap, FS&& on_sample) {
    constexpr int K = (kDeg + 1) * (kDeg + 1);
    const int C = 1 + 3 * K + a.E;
    const double(&o)[3] = row.o;
    const double(&d)[3] = row.d;
    const double tn = row.tn, dt = row.dt;
    {
        const int n = row.n;
        const double stepw = dt * row.len;
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
            typename Store::Tap tap;
            if (!a.store.present(c, a.n, tap)) {
                if (Store::kBricks && !a.store.jumps()) {  // an absent brick without jumps: one sigma tap of value 0
                    on_tap();
                    ++k;
                    continue;
                }
                // every cell of this brick has corners <= 0 or NaN only: skip to the last lattice point still in it
                const int b[3] = {c[0] >> kShift, c[1] >> kShift, c[2] >> kShift};
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
            // ---- the trilinear tap: weights (wx wy) wz, corners in the order i, j, k, low corner first
            double w[8];
            a.store.locate(c, a.n, C, tap);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int qi = q >> 2, qj = (q >> 1) & 1, qk = q & 1;
                w[q] = ((qi ? f[0] : 1.0 - f[0]) * (qj ? f[1] : 1.0 - f[1])) * (qk ? f[2] : 1.0 - f[2]);
            }
            on_tap();
            double sigma = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) sigma = sigma + w[q] * a.store.value(tap, q, 0);
            if (!(sigma > 0.0)) {
                ++k;
                continue;
            }
            double col[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < K; ++kk) {
                double tri[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < 8; ++q) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) tri[ch] = tri[ch] + w[q] * a.store.value(tap, q, 1 + 3 * kk + ch);
                }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) col[ch] = col[ch] + Y[kk] * tri[ch];
            }
            const double alpha = 1.0 - exp(-sigma * stepw);
            const double wgt = T * alpha;
            on_sample(c, w, tap, t, col, alpha, wgt, T);
            T = T * (1.0 - alpha);
            if (T < a.t_min) break;
            ++k;
        }
    }
}

template <class Store, int kDeg, int kEmax>
__global__ __launch_bounds__(kThreads) void k_volume_march(MarchRows<Store> a, MarchOut out) {
    constexpr int K = (kDeg + 1) * (kDeg + 1);
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= a.R) return;
    const Row row = load_row(a, r);
    double rgb[3] = {0.0, 0.0, 0.0}, at[kEmax > 0 ? kEmax : 1], acc = 0.0, wt = 0.0;
#pragma unroll
    for (int e = 0; e < kEmax; ++e) at[e] = 0.0;
    float depth = 0.f;
    int n_sigma = 0, n_colour = 0;
    if (row.valid) {
        double Y[K];
        sh_basis<kDeg>(row.d[0] / row.len, row.d[1] / row.len, row.d[2] / row.len, Y);
        march_row<kDeg>(
            a, row, Y, [&] { ++n_sigma; },
            [&](const int(&)[3], const double(&w)[8], const typename Store::Tap& tap, double t, const double(&s)[3], double,
                double wgt, double) {
                ++n_colour;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) rgb[ch] = rgb[ch] + wgt * (s[ch] > 0.0 ? s[ch] : 0.0);
#pragma unroll
                for (int e = 0; e < kEmax; ++e) {
                    if (e < a.E) {
                        double tri = 0.0;
#pragma unroll
                        for (int q = 0; q < 8; ++q) tri = tri + w[q] * a.store.value(tap, q, 1 + 3 * K + e);
                        at[e] = at[e] + wgt * tri;
                    }
                }
                acc = acc + wgt;
                wt = wt + wgt * t;
            });
        double q = wt / acc;
        if (q != q) q = 0.0;
        q = q > row.tn ? q : row.tn;
        // Degree 0 reads `far` again (volatile, or the compiler keeps the first load live) so that it is not carried through
        // the loop: the same value, two VGPRs fewer.  It holds the instances with attributes at 167 / 167 / 155 VGPRs (dense,
        // fp32, fp16 bricks), three waves per SIMD; without it the dense and the fp32-brick one take 169 and lose a wave.
        // The allocator decides this, not the language: after a compiler change, check those numbers in the resource report.
        const double tf = kDeg == 0 ? (double)*(const volatile float*)(a.far + r) : row.tf;
        q = q < tf ? q : tf;
        depth = (float)q;
    }
    if (out.rgb) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out.rgb[3 * r + ch] = (float)rgb[ch];
    }
    if (out.depth) out.depth[r] = depth;
    if (out.acc) out.acc[r] = (float)acc;
    if (out.taps) out.taps[2 * r] = n_sigma, out.taps[2 * r + 1] = n_colour;
    if (kEmax > 0 && out.attrs) {
#pragma unroll
        for (int e = 0; e < kEmax; ++e)
            if (e < a.E) out.attrs[(int64_t)a.E * r + e] = (float)at[e];
    }
}

// ---------------------------------------------------------------------------------------------------------- gradients
// The reverse of the compositing sweep (header, "radiance volume: gradients"): one ray per thread as in the forward, two
// runs of march_row.  Pass 1 sums U = sum wgt u over the row; pass 2 carries the prefix P, so that U - P is what the
// samples behind this one still add, and scatters 8 (1 + 3 K) contributions per sample as 64-bit integers of `quantum`:
// integer addition is associative, so sums depends on no order.  One vector atomic per non-zero contribution, relaxed, at
// agent scope; a thread's contributions of one sample go to 8 runs of 1 + 3 K consecutive sums, all distinct, so there is
// nothing to pre-sum within a sample, and summing across samples would need the cell's 8 (1 + 3 K) integers in registers.
__device__ __forceinline__ void scatter(const GradArgs& g, int64_t at, double x, bool& bad) {
    const double xq = x * g.inv_quantum;
    if (!(fabs(xq) < 4503599627370496.0)) {  // 2^52; a NaN or an infinity fails too
        bad = true;
        return;
    }
    const long long m = llrint(xq);  // round to nearest, ties to even
    if (m != 0) __hip_atomic_fetch_add(g.sums + at, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int kDeg>
__global__ __launch_bounds__(kThreads) void k_volume_march_bwd(MarchRows<DenseStore> a, GradArgs g) {
    constexpr int K = (kDeg + 1) * (kDeg + 1);
    constexpr int Cg = 1 + 3 * K;
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= a.R) return;
    const Row row = load_row(a, r);
    if (!row.valid) return;
    double gc[3] = {0.0, 0.0, 0.0}, ga = 0.0;
    if (g.g_rgb) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) gc[ch] = (double)g.g_rgb[3 * r + ch];
    }
    if (g.g_acc) ga = (double)g.g_acc[r];
    double Y[K];
    sh_basis<kDeg>(row.d[0] / row.len, row.d[1] / row.len, row.d[2] / row.len, Y);
    const double stepw = row.dt * row.len;
    auto upstream = [&](const double(&s)[3]) -> double {
        const double c0 = s[0] > 0.0 ? s[0] : 0.0, c1 = s[1] > 0.0 ? s[1] : 0.0, c2 = s[2] > 0.0 ? s[2] : 0.0;
        return ((gc[0] * c0 + gc[1] * c1) + gc[2] * c2) + ga;
    };
    double U = 0.0;
    const auto no_tap = [] {};
    march_row<kDeg>(a, row, Y, no_tap,
                    [&](const int(&)[3], const double(&)[8], const DenseStore::Tap&, double, const double(&s)[3], double,
                        double wgt, double) { U = U + wgt * upstream(s); });
    double P = 0.0;
    bool bad = false;
    march_row<kDeg>(a, row, Y, no_tap,
                    [&](const int(&c)[3], const double(&w)[8], const DenseStore::Tap&, double, const double(&s)[3],
                        double alpha, double wgt, double T) {
                        const double u = upstream(s);
                        P = P + wgt * u;
                        const double Tn = T * (1.0 - alpha);
                        const double ds = stepw * (Tn * u - (U - P));
                        double gw[3];
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) gw[ch] = wgt * gc[ch];
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            // corner q of cell c: a vertex of the grid, c <= n - 2 on every axis
                            const int64_t v = ((int64_t)(c[0] + (q >> 2)) * a.n[1] + (c[1] + ((q >> 1) & 1))) * a.n[2] +
                                              (c[2] + (q & 1));
                            const int64_t at = v * Cg;
                            scatter(g, at, w[q] * ds, bad);
#pragma unroll
                            for (int kk = 0; kk < K; ++kk) {
#pragma unroll
                                for (int ch = 0; ch < 3; ++ch)
                                    if (s[ch] > 0.0) scatter(g, at + 1 + 3 * kk + ch, w[q] * (Y[kk] * gw[ch]), bad);
                            }
                        }
                    });
    if (bad) __hip_atomic_fetch_or(g.flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread per entry of grad [N, C]; the flag is read by every thread and reset, if asked, by a launch of its own after
__global__ __launch_bounds__(kCopyThreads) void k_volume_grad_finish(int64_t total, int C, int Cg, long long* __restrict__ sums,
                                                                     double quantum, const int32_t* __restrict__ flag,
                                                                     float* __restrict__ grad, int clear) {
    const int64_t i = (int64_t)blockIdx.x * kCopyThreads + threadIdx.x;
    if (i >= total) return;
    const int64_t v = i / C;
    const int ch = (int)(i - v * C);
    float out = 0.f;
    if (ch < Cg) {
        const int64_t at = v * Cg + ch;
        out = (float)((double)sums[at] * quantum);
        if (clear) sums[at] = 0;
    }
    grad[i] = *flag != 0 ? __builtin_nanf("") : out;
}

__global__ void k_volume_flag_reset(int32_t* flag) { *flag = 0; }

bool grid_ok(int nx, int ny, int nz) {
    return nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz < ((int64_t)1 << 31);
}

// the argument checks of every marcher, forward and reverse
bool rows_ok(int64_t R, int nx, int ny, int nz, int sh_degree, int E, const float (&lo)[3], const float (&st)[3], float step,
             float t_min) {
    bool ok = R >= 0 && R < ((int64_t)1 << 31) * kThreads && grid_ok(nx, ny, nz) && sh_degree >= 0 && sh_degree <= 2 &&
              E >= 0 && E <= PN_VOLUME_MAX_ATTR && step > 0.f && step < INFINITY && t_min >= 0.f && t_min < INFINITY;
    for (int x = 0; x < 3; ++x) ok = ok && lo[x] - lo[x] == 0.f && st[x] > 0.f && st[x] < INFINITY;
    return ok;
}

// a power of two in [2^-60, 1]
bool quantum_ok(double quantum) {
    int e = 0;
    return quantum >= 0x1p-60 && quantum <= 1.0 && frexp(quantum, &e) == 0.5;
}

// The MarchRows of every marcher, forward and reverse: the checks, then the block the kernels take.  `have`: the caller's
// own pointers (the store's, the workspace's) are there.  PN_OK with R == 0 leaves nothing to launch.
template <class Store>
int march_rows(MarchRows<Store>& a, const Store& store, bool have, int64_t R, int nx, int ny, int nz, int sh_degree, int E,
               float x0, float y0, float z0, float dx, float dy, float dz, const float* origins, const float* directions,
               const float* near, const float* far, float step, float t_min) {
    const float lo[3] = {x0, y0, z0}, st[3] = {dx, dy, dz};
    if (!rows_ok(R, nx, ny, nz, sh_degree, E, lo, st, step, t_min)) return PN_ERR_BAD_SHAPE;
    if (R == 0) return PN_OK;
    if (!have || !origins || !directions || !near || !far) return PN_ERR_NULL;
    a = {R, {nx, ny, nz}, E, store, {}, {}, origins, directions, near, far, (double)step, (double)t_min};
    for (int x = 0; x < 3; ++x) a.lo[x] = (double)lo[x], a.st[x] = (double)st[x];
    return PN_OK;
}

// the marchers are instances over the SH degree: launch(std::integral_constant<int, degree>) of a checked sh_degree
template <class F>
void by_degree(int sh_degree, F&& launch) {
    switch (sh_degree) {
        case 0: launch(std::integral_constant<int, 0>{}); break;
        case 1: launch(std::integral_constant<int, 1>{}); break;
        default: launch(std::integral_constant<int, 2>{}); break;
    }
}

// what pn_volume_march and pn_volume_march_sparse share
template <class Store>
int march(const Store& store, bool have_store, int64_t R, int nx, int ny, int nz, int sh_degree, int E, float x0, float y0,
          float z0, float dx, float dy, float dz, const float* origins, const float* directions, const float* near,
          const float* far, float step, float t_min, const MarchOut& out, void* stream) {
    MarchRows<Store> a;
    const int rc = march_rows(a, store, have_store, R, nx, ny, nz, sh_degree, E, x0, y0, z0, dx, dy, dz, origins, directions,
                              near, far, step, t_min);
    if (rc != PN_OK || R == 0) return rc;
    const dim3 grid(nblk(R, kThreads)), block(kThreads);
    by_degree(sh_degree, [&](auto deg) {
        if (E > 0 && out.attrs)
            hipLaunchKernelGGL((k_volume_march<Store, deg.value, PN_VOLUME_MAX_ATTR>), grid, block, 0, ST(stream), a, out);
        else
            hipLaunchKernelGGL((k_volume_march<Store, deg.value, 0>), grid, block, 0, ST(stream), a, out);
    });
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int64_t brick_count(int nx, int ny, int nz) { return (int64_t)bricks_along(nx) * bricks_along(ny) * bricks_along(nz); }

// the checks pack and unpack share; B 729 C < 2^40 keeps every value index far inside 64 bits
bool pool_ok(int nx, int ny, int nz, int channels, int64_t B) {
    if (!grid_ok(nx, ny, nz) || channels < 1 || channels > 65536 || B < 0) return false;
    return B <= brick_count(nx, ny, nz) && B * kBrickVerts * channels < ((int64_t)1 << 40);
}

}  // namespace

extern "C" {

int64_t pn_volume_bricks(int nx, int ny, int nz) {
    if (!grid_ok(nx, ny, nz)) return -1;
    return brick_count(nx, ny, nz);
}

int pn_volume_occupancy(int nx, int ny, int nz, int channels, const float* data, uint8_t* occupancy, void* stream) {
    if (!grid_ok(nx, ny, nz) || channels < 1) return PN_ERR_BAD_SHAPE;
    if (!data || !occupancy) return PN_ERR_NULL;
    const dim3 grid((unsigned)brick_count(nx, ny, nz)), block(kThreads);
    hipLaunchKernelGGL(k_volume_occupancy, grid, block, 0, ST(stream), nx, ny, nz, channels, data, bricks_along(ny),
                       bricks_along(nz), occupancy);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_volume_march(int64_t R, int nx, int ny, int nz, int sh_degree, int E, const float* data, const uint8_t* occupancy,
                    float x0, float y0, float z0, float dx, float dy, float dz, const float* origins,
                    const float* directions, const float* near, const float* far, float step, float t_min, float* rgb,
                    float* depth, float* acc, float* attrs, int32_t* taps, void* stream) {
    return march(DenseStore{data, occupancy}, data != nullptr, R, nx, ny, nz, sh_degree, E, x0, y0, z0, dx, dy, dz, origins,
                 directions, near, far, step, t_min, {rgb, depth, acc, attrs, taps}, stream);
}

int pn_volume_march_bwd(int64_t R, int nx, int ny, int nz, int sh_degree, int E, const float* data, const uint8_t* occupancy,
                        float x0, float y0, float z0, float dx, float dy, float dz, const float* origins,
                        const float* directions, const float* near, const float* far, float step, float t_min,
                        const float* g_rgb, const float* g_acc, double quantum, int64_t* sums, int32_t* flag, void* stream) {
    if (!quantum_ok(quantum)) return PN_ERR_BAD_SHAPE;
    MarchRows<DenseStore> a;
    const int rc = march_rows(a, DenseStore{data, occupancy}, data && sums && flag, R, nx, ny, nz, sh_degree, E, x0, y0, z0, dx,
                              dy, dz, origins, directions, near, far, step, t_min);
    if (rc != PN_OK || R == 0) return rc;
    const GradArgs g{g_rgb, g_acc, 1.0 / quantum, (long long*)sums, flag};
    const dim3 grid(nblk(R, kThreads)), block(kThreads);
    by_degree(sh_degree,
              [&](auto deg) { hipLaunchKernelGGL(k_volume_march_bwd<deg.value>, grid, block, 0, ST(stream), a, g); });
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_volume_grad_finish(int64_t N, int C, int Cg, int64_t* sums, double quantum, int32_t* flag, float* grad, int clear,
                          void* stream) {
    if (N < 0 || N >= ((int64_t)1 << 31) || Cg < 1 || C < Cg || C > 1 + 27 + PN_VOLUME_MAX_ATTR || !quantum_ok(quantum))
        return PN_ERR_BAD_SHAPE;
    if (N == 0) return PN_OK;
    if (!sums || !flag || !grad) return PN_ERR_NULL;
    const int64_t total = N * C;
    hipLaunchKernelGGL(k_volume_grad_finish, dim3(nblk(total, kCopyThreads)), dim3(kCopyThreads), 0, ST(stream), total, C, Cg,
                       (long long*)sums, quantum, flag, grad, clear);
    PN_CHECK_LAUNCH();
    if (clear) {
        hipLaunchKernelGGL(k_volume_flag_reset, dim3(1), dim3(1), 0, ST(stream), flag);
        PN_CHECK_LAUNCH();
    }
    return PN_OK;
}

int pn_volume_pack(int nx, int ny, int nz, int channels, const int32_t* table, int64_t B, const float* data,
                   const float* rows, int64_t M, const int32_t* vertex_row, int half, void* pool, void* stream) {
    const bool dense = data != nullptr, by_rows = rows != nullptr || vertex_row != nullptr;
    if (!pool_ok(nx, ny, nz, channels, B) || M < 0 || (dense && by_rows)) return PN_ERR_BAD_SHAPE;
    if (!table || !(dense || by_rows) || (by_rows && (!vertex_row || (M > 0 && !rows)))) return PN_ERR_NULL;
    if (B == 0) return PN_OK;
    if (!pool) return PN_ERR_NULL;
    const int nby = bricks_along(ny), nbz = bricks_along(nz);
    const dim3 grid((unsigned)brick_count(nx, ny, nz)), block(kCopyThreads);
    if (half)
        hipLaunchKernelGGL(k_volume_pack<_Float16>, grid, block, 0, ST(stream), nx, ny, nz, channels, table, B, data, rows, M,
                           vertex_row, nby, nbz, (_Float16*)pool);
    else
        hipLaunchKernelGGL(k_volume_pack<float>, grid, block, 0, ST(stream), nx, ny, nz, channels, table, B, data, rows, M,
                           vertex_row, nby, nbz, (float*)pool);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_volume_unpack(int nx, int ny, int nz, int channels, const int32_t* table, int64_t B, const void* pool, int half,
                     float* data, void* stream) {
    if (!pool_ok(nx, ny, nz, channels, B)) return PN_ERR_BAD_SHAPE;
    if (!table || !data || (B > 0 && !pool)) return PN_ERR_NULL;
    const int nbx = bricks_along(nx), nby = bricks_along(ny), nbz = bricks_along(nz);
    const dim3 grid(nblk((int64_t)nx * ny * nz, kCopyThreads)), block(kCopyThreads);
    if (half)
        hipLaunchKernelGGL(k_volume_unpack<_Float16>, grid, block, 0, ST(stream), nx, ny, nz, channels, table, B,
                           (const _Float16*)pool, nbx, nby, nbz, data);
    else
        hipLaunchKernelGGL(k_volume_unpack<float>, grid, block, 0, ST(stream), nx, ny, nz, channels, table, B,
                           (const float*)pool, nbx, nby, nbz, data);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_volume_march_sparse(int64_t R, int nx, int ny, int nz, int sh_degree, int E, const int32_t* table, const void* pool,
                           int half, int skip, float x0, float y0, float z0, float dx, float dy, float dz,
                           const float* origins, const float* directions, const float* near, const float* far, float step,
                           float t_min, float* rgb, float* depth, float* acc, float* attrs, int32_t* taps, void* stream) {
    const auto go = [&](auto store) {
        return march(store, table != nullptr, R, nx, ny, nz, sh_degree, E, x0, y0, z0, dx, dy, dz, origins, directions, near,
                     far, step, t_min, {rgb, depth, acc, attrs, taps}, stream);
    };
    return half ? go(BrickStore<_Float16>{table, (const _Float16*)pool, skip})
                : go(BrickStore<float>{table, (const float*)pool, skip});
}

}  // extern "C"
