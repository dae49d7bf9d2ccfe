// pn_meshops.hip — cleaning and simplifying triangle meshes (gfx950): connected components of a mesh (union-find over vertex
// indices, the loop of pn_unionfind.h), the record of every component, and quadric vertex clustering (Lindstrom 2000 on
// Rossignac-Borrel cells).  The conventions (cells, quadric, solve, summation orders) are stated term for term in
// include/panonerf_hip.h, section "mesh operations"; tests/_meshops_ref.py follows them operation for operation.
//
// Every floating-point value is computed in fp64 on the fp32 inputs in an order that depends on the input alone and is
// rounded once; the only atomics are 32-bit integer ones (atomicMin on the parent array, atomicAdd on a vertex count),
// whose results do not depend on the order in which they land.  Two calls on the same inputs give the same bits.  Sorting,
// scanning and compaction are the caller's (torch), as pn_bvh.hip and pn_emitters.hip leave them.
//
// Every kernel checks the indices it reads (faces against V, order entries against their array) before it uses them, so
// a malformed input is skipped, never followed.
#include "pn_common.h"
#include "pn_unionfind.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / PN_WAVE;

// the three corners of face f, or false where one is outside [0, V)
__device__ __forceinline__ bool corners(const int32_t* faces, int64_t f, int64_t V, int32_t& a, int32_t& b, int32_t& c) {
    a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    return a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;
}

// ---- 0. validation: bad[0] = 1 where a coordinate is not finite, bad[1] = 1 where a face index is outside [0, V) ------
__global__ __launch_bounds__(kThreads) void k_mesh_check(int64_t V, int64_t F, const float* verts, const int32_t* faces,
                                                        int32_t* bad) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (verts && e < 3 * V && !isfinite(verts[e])) bad[0] = 1;  // every writer stores the same value
    if (e < 3 * F && (faces[e] < 0 || faces[e] >= V)) bad[1] = 1;
}

// ---- 1. components: union-find over vertex indices ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_comp_init(int64_t V, int32_t* parent) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v < V) parent[v] = -1;
}

// a vertex some face uses is its own parent (P1 of pn_unionfind.h); every writer of an element stores the same value
__global__ __launch_bounds__(kThreads) void k_comp_mark(int64_t F, int64_t V, const int32_t* faces, int32_t* parent) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    int32_t a, b, c;
    if (!corners(faces, f, V, a, b, c)) return;
    parent[a] = a, parent[b] = b, parent[c] = c;
}

__global__ __launch_bounds__(kThreads) void k_comp_union(int64_t F, int64_t V, const int32_t* faces, int32_t* parent) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    int32_t a, b, c;
    if (!corners(faces, f, V, a, b, c)) return;
    unite(parent, a, b);
    unite(parent, b, c);
}

// roots[v] = the root of vertex v (-1: no face uses it), flags[v] = 1 at a root.  parent is only read here.
__global__ __launch_bounds__(kThreads) void k_comp_flatten(int64_t V, const int32_t* parent, int32_t* roots, int32_t* flags) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    int32_t i = (int32_t)v;
    int32_t q = parent[i];
    if (q >= 0) {
        while (q != i) {  // (P1): strictly down to the root
            i = q;
            q = parent[i];
        }
    }
    roots[v] = q;
    flags[v] = q == (int32_t)v ? 1 : 0;
}

// vertex_label[v] = prefix[root] - 1 (prefix = the inclusive count of flags), face_label[f] = the label of its first corner
__global__ __launch_bounds__(kThreads) void k_comp_labels(int64_t V, int64_t F, const int32_t* faces, const int32_t* roots,
                                                         const int32_t* prefix, int32_t* vertex_label, int32_t* face_label,
                                                         int32_t* count) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e < V) {
        const int32_t r = roots[e];
        vertex_label[e] = (r >= 0 && r < V) ? prefix[r] - 1 : -1;
        if (e == V - 1) count[0] = prefix[e];
    }
    if (e < F) {
        int32_t a, b, c, lab = -1;
        if (corners(faces, e, V, a, b, c)) {
            const int32_t r = roots[a];
            if (r >= 0 && r < V) lab = prefix[r] - 1;
        }
        face_label[e] = lab;
    }
}

// nverts[l] += the number of vertices labelled l.  Integer counts: the same whatever the order.  The lanes of a wave that
// hold the same label add their count with ONE atomic (the vertices of a mesh are mostly one component: one atomic per
// vertex on one address would serialise the whole pass), so every lane stays in the loop until the wave is done.
__global__ __launch_bounds__(kThreads) void k_comp_vcount(int64_t V, int64_t C, const int32_t* vertex_label, int32_t* nverts) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t l = v < V ? vertex_label[v] : -1;
    bool todo = l >= 0 && l < C;
    for (;;) {
        const unsigned long long open = __ballot(todo);
        if (!open) break;
        const int leader = __ffsll((long long)open) - 1;
        const int32_t ll = __shfl(l, leader, 64);
        const bool same = todo && l == ll;
        const unsigned long long group = __ballot(same);
        if (lane == leader) atomicAdd(nverts + ll, (int32_t)__popcll(group));
        if (same) todo = false;
    }
}

constexpr int kChunk = 4096;  // faces per workgroup of the component records: 16 per thread
constexpr int kPart = 10;     // doubles per partial: count, area, volume, -, min[3], max[3] (fp32 values, held exactly)

struct StatsArgs {
    int64_t V, F, C, B;
    const float* verts;
    const int32_t* faces;
    const int64_t *order, *starts, *chunk_starts;
    double* work;
    int32_t* nfaces;
    float *area, *volume, *bbox;
};

// Pass 1, one workgroup of 256 threads per chunk.  order[starts[c] .. starts[c + 1]) are the faces of component c in
// ascending order; chunk j of it is the elements [4096 j, 4096 (j + 1)) of that list, and workgroup chunk_starts[c] + j
// takes it (chunk_starts[c + 1] - chunk_starts[c] = ceil(n_c / 4096); the workgroup finds its c by bisection).  Thread t
// takes elements t, t + 256, ... of the chunk in order, the lanes of a wave meet in the xor butterfly 32 .. 1, thread 0
// adds the four waves in order and writes the chunk's partial.  One visit of every face: the work does not grow as C x F,
// and a component of millions of faces is spread over the whole device.
__global__ __launch_bounds__(kThreads) void k_comp_stats(StatsArgs s) {
    const int64_t b = blockIdx.x;
    if (b >= s.B || b >= s.chunk_starts[s.C]) return;
    int64_t c = 0, top = s.C;  // the largest c with chunk_starts[c] <= b
    while (top - c > 1) {
        const int64_t mid = (c + top) >> 1;
        if (s.chunk_starts[mid] <= b) c = mid; else top = mid;
    }
    const int64_t j = b - s.chunk_starts[c];
    int64_t end = s.starts[c + 1];
    end = end < 0 ? 0 : (end > s.F ? s.F : end);
    int64_t lo = s.starts[c] + j * kChunk;
    if (j < 0 || lo < 0 || lo > end) lo = end;
    const int64_t hi = lo + kChunk < end ? lo + kChunk : end;
    double n = 0.0, ar = 0.0, vol = 0.0;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t k = lo + threadIdx.x; k < hi; k += kThreads) {
        const int64_t f = s.order[k];
        if (f < 0 || f >= s.F) continue;
        int32_t ia, ib, ic;
        if (!corners(s.faces, f, s.V, ia, ib, ic)) continue;
        const float *pa = s.verts + 3 * (int64_t)ia, *pb = s.verts + 3 * (int64_t)ib, *pc = s.verts + 3 * (int64_t)ic;
        const double a0 = pa[0], a1 = pa[1], a2 = pa[2], b0 = pb[0], b1 = pb[1], b2 = pb[2], c0 = pc[0], c1 = pc[1], c2 = pc[2];
        const double u0 = b0 - a0, u1 = b1 - a1, u2 = b2 - a2, w0 = c0 - a0, w1 = c1 - a1, w2 = c2 - a2;
        const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
        ar += sqrt((n0 * n0 + n1 * n1) + n2 * n2);
        const double x0 = b1 * c2 - b2 * c1, x1 = b2 * c0 - b0 * c2, x2 = b0 * c1 - b1 * c0;
        vol += (a0 * x0 + a1 * x1) + a2 * x2;
        n += 1.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            mn[q] = fminf(mn[q], fminf(pa[q], fminf(pb[q], pc[q])));
            mx[q] = fmaxf(mx[q], fmaxf(pa[q], fmaxf(pb[q], pc[q])));
        }
    }
    n = wave_sum(n), ar = wave_sum(ar), vol = wave_sum(vol);
#pragma unroll
    for (int q = 0; q < 3; ++q)
        for (int o = 32; o > 0; o >>= 1) {
            mn[q] = fminf(mn[q], __shfl_xor(mn[q], o, 64));
            mx[q] = fmaxf(mx[q], __shfl_xor(mx[q], o, 64));
        }
    __shared__ double red[3][kWaves];
    __shared__ float box[6][kWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wv] = n, red[1][wv] = ar, red[2][wv] = vol;
#pragma unroll
        for (int q = 0; q < 3; ++q) box[q][wv] = mn[q], box[3 + q][wv] = mx[q];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kWaves; ++w) {
        n += red[0][w], ar += red[1][w], vol += red[2][w];
#pragma unroll
        for (int q = 0; q < 3; ++q) mn[q] = fminf(mn[q], box[q][w]), mx[q] = fmaxf(mx[q], box[3 + q][w]);
    }
    double* part = s.work + kPart * b;
    part[0] = n, part[1] = ar, part[2] = vol, part[3] = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) part[4 + q] = mn[q], part[7 + q] = mx[q];
}

// Pass 2, one thread per component: its chunks' partials in ascending chunk order, sequentially, from 0.0
__global__ __launch_bounds__(kThreads) void k_comp_stats_final(StatsArgs s) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= s.C) return;
    int64_t lo = s.chunk_starts[c], hi = s.chunk_starts[c + 1];
    lo = lo < 0 ? 0 : (lo > s.B ? s.B : lo);
    hi = hi < lo ? lo : (hi > s.B ? s.B : hi);
    double n = 0.0, ar = 0.0, vol = 0.0;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t b = lo; b < hi; ++b) {
        const double* part = s.work + kPart * b;
        n += part[0], ar += part[1], vol += part[2];
#pragma unroll
        for (int q = 0; q < 3; ++q) mn[q] = fminf(mn[q], (float)part[4 + q]), mx[q] = fmaxf(mx[q], (float)part[7 + q]);
    }
    if (n == 0.0) return;  // an empty row stays as the caller zeroed it
    s.nfaces[c] = (int32_t)n;
    s.area[c] = (float)(ar / 2.0);
    s.volume[c] = (float)(vol / 6.0);
#pragma unroll
    for (int q = 0; q < 3; ++q) s.bbox[6 * c + q] = mn[q], s.bbox[6 * c + 3 + q] = mx[q];
}

// ---- 2. quadric vertex clustering -----------------------------------------------------------------------------------
struct Cells {
    float lo[3], cell;
    int64_t n[3];
};

// floor((double(v) - double(lo)) / double(cell)) clamped to [0, n - 1]; the clamp runs in fp64, before the conversion
__device__ __forceinline__ int64_t cell_index(float v, float lo, float cell, int64_t n) {
    double q = floor(((double)v - (double)lo) / (double)cell);
    const double top = (double)(n - 1);
    if (!(q >= 0.0)) q = 0.0;
    if (q > top) q = top;
    return (int64_t)q;
}

__global__ __launch_bounds__(kThreads) void k_cluster_keys(int64_t V, const float* verts, Cells g, int64_t* keys) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    const int64_t ix = cell_index(verts[3 * v], g.lo[0], g.cell, g.n[0]);
    const int64_t iy = cell_index(verts[3 * v + 1], g.lo[1], g.cell, g.n[1]);
    const int64_t iz = cell_index(verts[3 * v + 2], g.lo[2], g.cell, g.n[2]);
    keys[v] = (ix * g.n[1] + iy) * g.n[2] + iz;
}

constexpr int64_t kNoFace = 0x7fffffffffffffffLL;

// out[f] = the face through the vertex -> cluster rank; fkey[f] = (s0 << 42) | (s1 << 21) | s2 of its sorted triple, or
// kNoFace (sorts last) where two corners fall into one cluster or an index is out of range
__global__ __launch_bounds__(kThreads) void k_cluster_faces(int64_t F, int64_t V, int64_t K, const int32_t* faces,
                                                           const int32_t* rank, int32_t* out, int64_t* fkey) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    int32_t a, b, c;
    int64_t key = kNoFace;
    int32_t r0 = -1, r1 = -1, r2 = -1;
    if (corners(faces, f, V, a, b, c)) {
        r0 = rank[a], r1 = rank[b], r2 = rank[c];
        const bool ok = r0 >= 0 && r1 >= 0 && r2 >= 0 && r0 < K && r1 < K && r2 < K;
        if (ok && r0 != r1 && r1 != r2 && r0 != r2) {
            int64_t s0 = r0, s1 = r1, s2 = r2, t;
            if (s0 > s1) t = s0, s0 = s1, s1 = t;
            if (s1 > s2) t = s1, s1 = s2, s2 = t;
            if (s0 > s1) t = s0, s0 = s1, s1 = t;
            key = (s0 << 42) | (s1 << 21) | s2;
        }
    }
    out[3 * f] = r0, out[3 * f + 1] = r1, out[3 * f + 2] = r2;
    fkey[f] = key;
}

struct SolveArgs {
    int64_t K, V, F;
    const float* verts;
    const int32_t* faces;
    const float *normals, *colors;
    Cells g;
    const int64_t *ckeys, *vorder, *vstarts, *iorder, *istarts;
    double lam;
    float *out_v, *out_n, *out_c;
    uint8_t* flags;
};

// One thread per cluster, everything sequential in the order of the header: the vertices of the cluster in ascending
// index, then its (face, corner) incidences in ascending 3 f + corner, then the LDL^T solve.  Twelve fp64 accumulators
// and the 3 x 3 system live in registers.
__global__ __launch_bounds__(kThreads) void k_cluster_solve(SolveArgs s) {
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= s.K) return;
    const int64_t key = s.ckeys[k];
    const int64_t iz = key % s.g.n[2], iy = (key / s.g.n[2]) % s.g.n[1], ix = key / (s.g.n[2] * s.g.n[1]);
    const double cell = (double)s.g.cell;
    const double c0 = (double)s.g.lo[0] + ((double)ix + 0.5) * cell;
    const double c1 = (double)s.g.lo[1] + ((double)iy + 0.5) * cell;
    const double c2 = (double)s.g.lo[2] + ((double)iz + 0.5) * cell;

    int64_t lo = s.vstarts[k], hi = s.vstarts[k + 1];
    lo = lo < 0 ? 0 : (lo > s.V ? s.V : lo);
    hi = hi < lo ? lo : (hi > s.V ? s.V : hi);
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, h0 = 0.0, h1 = 0.0, h2 = 0.0, cnt = 0.0;
    for (int64_t j = lo; j < hi; ++j) {
        const int64_t v = s.vorder[j];
        if (v < 0 || v >= s.V) continue;
        m0 += (double)s.verts[3 * v] - c0, m1 += (double)s.verts[3 * v + 1] - c1, m2 += (double)s.verts[3 * v + 2] - c2;
        if (s.normals) g0 += (double)s.normals[3 * v], g1 += (double)s.normals[3 * v + 1], g2 += (double)s.normals[3 * v + 2];
        if (s.colors) h0 += (double)s.colors[3 * v], h1 += (double)s.colors[3 * v + 1], h2 += (double)s.colors[3 * v + 2];
        cnt += 1.0;
    }
    const double xb0 = m0 / cnt, xb1 = m1 / cnt, xb2 = m2 / cnt;  // cnt = 0 cannot be: a cluster is an occupied cell
    if (s.out_n) {
        const double a0 = g0 / cnt, a1 = g1 / cnt, a2 = g2 / cnt;
        const double nn = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
        const bool ok = nn >= 1e-12;
        s.out_n[3 * k] = ok ? (float)(a0 / nn) : 0.f;
        s.out_n[3 * k + 1] = ok ? (float)(a1 / nn) : 0.f;
        s.out_n[3 * k + 2] = ok ? (float)(a2 / nn) : 0.f;
    }
    if (s.out_c) s.out_c[3 * k] = (float)(h0 / cnt), s.out_c[3 * k + 1] = (float)(h1 / cnt), s.out_c[3 * k + 2] = (float)(h2 / cnt);

    int64_t il = s.istarts[k], ih = s.istarts[k + 1];
    const int64_t N = 3 * s.F;
    il = il < 0 ? 0 : (il > N ? N : il);
    ih = ih < il ? il : (ih > N ? N : ih);
    double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int64_t j = il; j < ih; ++j) {
        const int64_t i = s.iorder[j];
        if (i < 0 || i >= N) continue;
        int32_t ia, ib, ic;
        if (!corners(s.faces, i / 3, s.V, ia, ib, ic)) continue;
        const float *pa = s.verts + 3 * (int64_t)ia, *pb = s.verts + 3 * (int64_t)ib, *pc = s.verts + 3 * (int64_t)ic;
        const double a0 = pa[0], a1 = pa[1], a2 = pa[2];
        const double u0 = (double)pb[0] - a0, u1 = (double)pb[1] - a1, u2 = (double)pb[2] - a2;
        const double w0 = (double)pc[0] - a0, w1 = (double)pc[1] - a1, w2 = (double)pc[2] - a2;
        const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
        const double d = -((n0 * (a0 - c0) + n1 * (a1 - c1)) + n2 * (a2 - c2));
        A00 += n0 * n0, A01 += n0 * n1, A02 += n0 * n2, A11 += n1 * n1, A12 += n1 * n2, A22 += n2 * n2;
        b0 += n0 * d, b1 += n1 * d, b2 += n2 * d;
    }
    const double t = (A00 + A11) + A22;
    double x0 = xb0, x1 = xb1, x2 = xb2;
    uint8_t flag = 2;  // no quadric
    if (t != 0.0) {
        const double sh = s.lam * t;
        const double q00 = A00 + sh, q11 = A11 + sh, q22 = A22 + sh;
        const double r0 = sh * xb0 - b0, r1 = sh * xb1 - b1, r2 = sh * xb2 - b2;
        // LDL^T of the symmetric 3 x 3 system, then the two triangular solves
        const double l10 = A01 / q00, l20 = A02 / q00;
        const double d1 = q11 - l10 * A01;
        const double u12 = A12 - l20 * A01;
        const double l21 = u12 / d1;
        const double d2 = (q22 - l20 * A02) - l21 * u12;
        const double y1 = r1 - l10 * r0;
        const double y2 = (r2 - l20 * r0) - l21 * y1;
        const double z2 = y2 / d2;
        const double z1 = y1 / d1 - l21 * z2;
        const double z0 = (r0 / q00 - l10 * z1) - l20 * z2;
        const double half = cell * 0.5;
        const bool ok = isfinite(z0) && isfinite(z1) && isfinite(z2) && fabs(z0) <= half && fabs(z1) <= half && fabs(z2) <= half;
        if (ok) x0 = z0, x1 = z1, x2 = z2;
        flag = ok ? 0 : 1;
    }
    s.out_v[3 * k] = (float)(c0 + x0), s.out_v[3 * k + 1] = (float)(c1 + x1), s.out_v[3 * k + 2] = (float)(c2 + x2);
    s.flags[k] = flag;
}

constexpr int64_t kMaxIndex = (int64_t)1 << 31;  // int32 indices

int check_mesh(int64_t V, int64_t F) { return (V < 0 || F < 0 || V >= kMaxIndex || F >= kMaxIndex) ? PN_ERR_BAD_SHAPE : PN_OK; }

int check_cells(float lox, float loy, float loz, float cell, int64_t nx, int64_t ny, int64_t nz) {
    if (!(isfinite(lox) && isfinite(loy) && isfinite(loz) && isfinite(cell) && cell > 0.f)) return PN_ERR_BAD_SHAPE;
    if (nx < 1 || ny < 1 || nz < 1) return PN_ERR_BAD_SHAPE;
    const int64_t top = 0x7fffffffffffffffLL;
    if (nx > top / ny || nx * ny > top / nz) return PN_ERR_BAD_SHAPE;  // the key does not fit 63 bits
    return PN_OK;
}

}  // namespace

extern "C" {

int pn_mesh_check(int64_t V, int64_t F, const float* vertices, const int32_t* faces, int32_t* bad, void* stream) {
    int st = check_mesh(V, F);
    if (st != PN_OK) return st;
    if (!bad || (F > 0 && !faces)) return PN_ERR_NULL;  // vertices = NULL: only the faces are judged
    if (hipMemsetAsync(bad, 0, 2 * sizeof(int32_t), ST(stream)) != hipSuccess) return PN_ERR_HIP;
    const int64_t n = 3 * (V > F ? V : F);
    if (n == 0) return PN_OK;
    hipLaunchKernelGGL(k_mesh_check, dim3(nblk(n, kThreads)), dim3(kThreads), 0, ST(stream), V, F, vertices, faces, bad);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_mesh_components(int64_t V, int64_t F, const int32_t* faces, int32_t* parent, int32_t* roots, int32_t* flags,
                       void* stream) {
    int st = check_mesh(V, F);
    if (st != PN_OK) return st;
    if (V == 0) return PN_OK;
    if (!parent || !roots || !flags || (F > 0 && !faces)) return PN_ERR_NULL;
    const dim3 gv(nblk(V, kThreads)), gf(nblk(F, kThreads)), block(kThreads);
    hipLaunchKernelGGL(k_comp_init, gv, block, 0, ST(stream), V, parent);
    PN_CHECK_LAUNCH();
    if (F > 0) {
        hipLaunchKernelGGL(k_comp_mark, gf, block, 0, ST(stream), F, V, faces, parent);
        PN_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_comp_union, gf, block, 0, ST(stream), F, V, faces, parent);
        PN_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_comp_flatten, gv, block, 0, ST(stream), V, parent, roots, flags);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_mesh_labels(int64_t V, int64_t F, const int32_t* faces, const int32_t* roots, const int32_t* prefix,
                   int32_t* vertex_label, int32_t* face_label, int32_t* count, void* stream) {
    int st = check_mesh(V, F);
    if (st != PN_OK) return st;
    if (V == 0) return F == 0 ? PN_OK : PN_ERR_BAD_SHAPE;
    if (!roots || !prefix || !vertex_label || !count || (F > 0 && (!faces || !face_label))) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_comp_labels, dim3(nblk(V > F ? V : F, kThreads)), dim3(kThreads), 0, ST(stream), V, F, faces, roots,
                       prefix, vertex_label, face_label, count);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_mesh_component_stats(int64_t V, int64_t F, int64_t C, const float* vertices, const int32_t* faces,
                            const int64_t* order, const int64_t* starts, const int64_t* chunk_starts, int64_t B,
                            double* work, const int32_t* vertex_label, int32_t* nfaces, int32_t* nverts, float* area,
                            float* volume, float* bbox, void* stream) {
    int st = check_mesh(V, F);
    if (st != PN_OK) return st;
    if (C < 0 || C > V || B < 0 || B >= kMaxIndex) return PN_ERR_BAD_SHAPE;
    if (C == 0) return PN_OK;
    if (!vertices || !faces || !order || !starts || !chunk_starts || !vertex_label || !nfaces || !nverts || !area || !volume ||
        !bbox || (B > 0 && !work))
        return PN_ERR_NULL;
    hipLaunchKernelGGL(k_comp_vcount, dim3(nblk(V, kThreads)), dim3(kThreads), 0, ST(stream), V, C, vertex_label, nverts);
    PN_CHECK_LAUNCH();
    if (B == 0) return PN_OK;
    StatsArgs a{V, F, C, B, vertices, faces, order, starts, chunk_starts, work, nfaces, area, volume, bbox};
    hipLaunchKernelGGL(k_comp_stats, dim3((unsigned)B), dim3(kThreads), 0, ST(stream), a);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_comp_stats_final, dim3(nblk(C, kThreads)), dim3(kThreads), 0, ST(stream), a);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_cluster_keys(int64_t V, const float* vertices, float lox, float loy, float loz, float cell, int64_t nx, int64_t ny,
                    int64_t nz, int64_t* keys, void* stream) {
    int st = check_mesh(V, 0);
    if (st != PN_OK) return st;
    st = check_cells(lox, loy, loz, cell, nx, ny, nz);
    if (st != PN_OK) return st;
    if (V == 0) return PN_OK;
    if (!vertices || !keys) return PN_ERR_NULL;
    const Cells g{{lox, loy, loz}, cell, {nx, ny, nz}};
    hipLaunchKernelGGL(k_cluster_keys, dim3(nblk(V, kThreads)), dim3(kThreads), 0, ST(stream), V, vertices, g, keys);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_cluster_faces(int64_t F, int64_t V, int64_t K, const int32_t* faces, const int32_t* rank, int32_t* out_faces,
                     int64_t* face_keys, void* stream) {
    int st = check_mesh(V, F);
    if (st != PN_OK) return st;
    if (K < 0 || K > V || K >= ((int64_t)1 << 21)) return PN_ERR_BAD_SHAPE;
    if (F == 0) return PN_OK;
    if (!faces || !rank || !out_faces || !face_keys) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_cluster_faces, dim3(nblk(F, kThreads)), dim3(kThreads), 0, ST(stream), F, V, K, faces, rank,
                       out_faces, face_keys);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_cluster_solve(int64_t K, int64_t V, int64_t F, const float* vertices, const int32_t* faces, const float* normals,
                     const float* colors, float lox, float loy, float loz, float cell, int64_t nx, int64_t ny, int64_t nz,
                     const int64_t* cluster_keys, const int64_t* vertex_order, const int64_t* vertex_starts,
                     const int64_t* incidence_order, const int64_t* incidence_starts, double lam, float* out_vertices,
                     float* out_normals, float* out_colors, uint8_t* flags, void* stream) {
    int st = check_mesh(V, F);
    if (st != PN_OK) return st;
    st = check_cells(lox, loy, loz, cell, nx, ny, nz);
    if (st != PN_OK) return st;
    if (K < 0 || K > V || !(lam >= 0.0 && isfinite(lam))) return PN_ERR_BAD_SHAPE;
    if (K == 0) return PN_OK;
    if (!vertices || !cluster_keys || !vertex_order || !vertex_starts || !incidence_starts || !out_vertices || !flags)
        return PN_ERR_NULL;
    if (F > 0 && (!faces || !incidence_order)) return PN_ERR_NULL;
    if ((out_normals && !normals) || (out_colors && !colors)) return PN_ERR_NULL;
    SolveArgs a{K, V, F, vertices, faces, normals, colors, Cells{{lox, loy, loz}, cell, {nx, ny, nz}}, cluster_keys,
                vertex_order, vertex_starts, incidence_order, incidence_starts, lam, out_vertices, out_normals, out_colors,
                flags};
    hipLaunchKernelGGL(k_cluster_solve, dim3(nblk(K, kThreads)), dim3(kThreads), 0, ST(stream), a);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

}  // extern "C"
