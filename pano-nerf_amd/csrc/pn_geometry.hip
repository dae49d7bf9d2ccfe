// pn_geometry.hip — export of the learned geometry (gfx950): the (mean, cov) rows of grid vertices, the activation
// epilogue of a field query (sigma, albedo, rgb, normal from the raw MLP outputs and d sigma / d mean), and marching
// tetrahedra over the Freudenthal (Kuhn) subdivision of a sigma volume.
//
// Marching tetrahedra in four stages (include/panonerf_hip.h states the contract):
//   classify  per vertex a 7-bit crossing mask of its 7 outgoing edges, per cell a triangle count (<= 12), and one
//             int64 sum per block of kItems elements;
//   scan      the block sums, exclusive, one workgroup per array (the two totals fall out);
//   fixup     per block, the exclusive scan of its elements plus its block offset -> int32 per element;
//   emit      vertices by edge (a thread per grid vertex), faces by cell (a thread per cell).
// No atomics and no communication between workgroups inside a launch: integer scans, identical output on every run.
#include "pn_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                    // elements per thread in the classify / fixup blocks
constexpr int kItems = kThreads * kPer;    // elements per block
constexpr int kScanThreads = 1024;

inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// edge offsets from the lower endpoint, in edge-id order: 3 axes, 3 face diagonals, the body diagonal
__constant__ int kOff[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
// the 6 tetrahedra of a cell: p -> p+e_a -> p+e_a+e_b -> p+(1,1,1) for (a, b) in xyz, xzy, yxz, yzx, zxy, zyx;
// kPar: orientation (sign of det(e_a, e_b, e_c)); odd tetrahedra emit each triangle with its last two vertices swapped
__constant__ int kPerm[6][2] = {{0, 1}, {0, 2}, {1, 0}, {1, 2}, {2, 0}, {2, 1}};
__constant__ int kPar[6] = {1, -1, -1, 1, 1, -1};
// tetrahedron edges (T_lo, T_hi): 0 (0,1), 1 (0,2), 2 (0,3), 3 (1,2), 4 (1,3), 5 (2,3)
__constant__ int kTetEdge[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// case = in(T0) | in(T1) << 1 | in(T2) << 2 | in(T3) << 3 -> triangles as tetrahedron-edge triples, wound for a
// positively oriented tetrahedron so that (v1 - v0) x (v2 - v0) points to the outside (the table of the header)
__constant__ int kTriCount[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
__constant__ int kTri[16][2][3] = {
    {{0, 0, 0}, {0, 0, 0}}, {{0, 1, 2}, {0, 0, 0}}, {{0, 4, 3}, {0, 0, 0}}, {{1, 2, 4}, {1, 4, 3}},
    {{1, 3, 5}, {0, 0, 0}}, {{0, 5, 2}, {0, 3, 5}}, {{0, 4, 5}, {0, 5, 1}}, {{2, 4, 5}, {0, 0, 0}},
    {{2, 5, 4}, {0, 0, 0}}, {{0, 1, 5}, {0, 5, 4}}, {{0, 5, 3}, {0, 2, 5}}, {{1, 5, 3}, {0, 0, 0}},
    {{1, 3, 4}, {1, 4, 2}}, {{0, 3, 4}, {0, 0, 0}}, {{0, 2, 1}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}};

struct Grid {
    int nx, ny, nz;
    int64_t nv, nc;  // vertices, cells
};

// inside <=> sigma > level (NaN: outside)
__device__ __forceinline__ bool inside(float s, float level) { return s > level; }

__device__ __forceinline__ int64_t vid(const Grid& g, int i, int j, int k) { return ((int64_t)i * g.ny + j) * g.nz + k; }

// corner bits of a cell: bit (dx*4 + dy*2 + dz)
__device__ __forceinline__ int cell_corners(const Grid& g, const float* sigma, float level, int i, int j, int k) {
    int bits = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int dx = c >> 2, dy = (c >> 1) & 1, dz = c & 1;
        bits |= (int)inside(sigma[vid(g, i + dx, j + dy, k + dz)], level) << c;
    }
    return bits;
}

// tetrahedron vertex q (0..3) of tetrahedron t as a cell-corner offset (dx, dy, dz)
__device__ __forceinline__ void tet_vertex(int t, int q, int d[3]) {
    d[0] = d[1] = d[2] = 0;
    if (q >= 1) d[kPerm[t][0]] = 1;
    if (q >= 2) d[kPerm[t][1]] = 1;
    if (q == 3) d[0] = d[1] = d[2] = 1;
}

__device__ __forceinline__ int tet_case(int corners, int t) {
    int cs = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int d[3];
        tet_vertex(t, q, d);
        cs |= ((corners >> (d[0] * 4 + d[1] * 2 + d[2])) & 1) << q;
    }
    return cs;
}

__device__ __forceinline__ void cell_of(const Grid& g, int64_t c, int& i, int& j, int& k) {
    const int64_t cy = g.ny - 1, cz = g.nz - 1;
    i = (int)(c / (cy * cz));
    const int64_t r = c - (int64_t)i * cy * cz;
    j = (int)(r / cz);
    k = (int)(r - (int64_t)j * cz);
}

__device__ __forceinline__ void vertex_of(const Grid& g, int64_t v, int& i, int& j, int& k) {
    const int64_t nyz = (int64_t)g.ny * g.nz;
    i = (int)(v / nyz);
    const int64_t r = v - (int64_t)i * nyz;
    j = (int)(r / g.nz);
    k = (int)(r - (int64_t)j * g.nz);
}

__device__ __forceinline__ int vertex_mask(const Grid& g, const float* sigma, float level, int64_t v) {
    int i, j, k;
    vertex_of(g, v, i, j, k);
    const bool a = inside(sigma[v], level);
    int mask = 0;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const int bi = i + kOff[s][0], bj = j + kOff[s][1], bk = k + kOff[s][2];
        if (bi < g.nx && bj < g.ny && bk < g.nz && inside(sigma[vid(g, bi, bj, bk)], level) != a) mask |= 1 << s;
    }
    return mask;
}

__device__ __forceinline__ int cell_tris(int corners) {
    int n = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) n += kTriCount[tet_case(corners, t)];
    return n;
}

// exclusive scan of one value per thread over the workgroup (kThreads lanes); returns the block total in *total
__device__ __forceinline__ int64_t block_exclusive(int64_t x, int64_t* total) {
    __shared__ int64_t wsum[kScanThreads / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int64_t inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int64_t before = 0, all = 0;
    for (int w = 0; w < nw; ++w) {
        const int64_t s = wsum[w];
        if (w < wv) before += s;
        all += s;
    }
    __syncthreads();  // wsum is reused by the next call
    *total = all;
    return before + inc - x;
}

// blocks [0, nbv): vertices; [nbv, nbv + nbc): cells
__global__ __launch_bounds__(kThreads) void k_mt_classify(Grid g, const float* sigma, float level, unsigned nbv,
                                                          uint8_t* vmask, uint8_t* ccnt, int64_t* vblk, int64_t* cblk) {
    const bool cells = blockIdx.x >= nbv;
    const int64_t b = cells ? blockIdx.x - nbv : blockIdx.x;
    const int64_t n = cells ? g.nc : g.nv;
    int64_t sum = 0;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const int64_t e = b * kItems + r * kThreads + threadIdx.x;
        if (e >= n) continue;
        if (cells) {
            int i, j, k;
            cell_of(g, e, i, j, k);
            const int cnt = cell_tris(cell_corners(g, sigma, level, i, j, k));
            ccnt[e] = (uint8_t)cnt;
            sum += cnt;
        } else {
            const int m = vertex_mask(g, sigma, level, e);
            vmask[e] = (uint8_t)m;
            sum += __popc(m);
        }
    }
    int64_t total;
    block_exclusive(sum, &total);
    if (threadIdx.x == 0) (cells ? cblk : vblk)[b] = total;
}

// block 0: vertex block sums, block 1: cell block sums -> exclusive, in place; totals[blockIdx.x] = the sum
__global__ __launch_bounds__(kScanThreads) void k_mt_scan_blocks(int64_t* vblk, int64_t nbv, int64_t* cblk, int64_t nbc,
                                                                 int64_t* totals) {
    int64_t* a = blockIdx.x ? cblk : vblk;
    const int64_t n = blockIdx.x ? nbc : nbv;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += kScanThreads) {
        const int64_t e = base + threadIdx.x;
        const int64_t x = e < n ? a[e] : 0;
        int64_t total;
        const int64_t ex = block_exclusive(x, &total);
        if (e < n) a[e] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kThreads) void k_mt_fixup(Grid g, unsigned nbv, const uint8_t* vmask, const uint8_t* ccnt,
                                                       const int64_t* vblk, const int64_t* cblk, int32_t* vscan,
                                                       int32_t* cscan) {
    const bool cells = blockIdx.x >= nbv;
    const int64_t b = cells ? blockIdx.x - nbv : blockIdx.x;
    const int64_t n = cells ? g.nc : g.nv;
    int64_t carry = (cells ? cblk : vblk)[b];
    for (int r = 0; r < kPer; ++r) {
        const int64_t e = b * kItems + r * kThreads + threadIdx.x;
        const int64_t x = e < n ? (cells ? (int64_t)ccnt[e] : (int64_t)__popc(vmask[e])) : 0;
        int64_t total;
        const int64_t ex = block_exclusive(x, &total);
        if (e < n) (cells ? cscan : vscan)[e] = (int32_t)(carry + ex);
        carry += total;
    }
}

struct Place {
    float o[3], d[3];  // world position of vertex (i, j, k) = o + (i, j, k) * d, per axis in fp32
};

__device__ __forceinline__ float axis_pos(const Place& p, int a, int i) { return p.o[a] + (float)i * p.d[a]; }

__global__ __launch_bounds__(kThreads) void k_mt_emit_vertices(Grid g, const float* sigma, float level,
                                                               const uint8_t* vmask, const int32_t* vscan,
                                                               int64_t max_vertices, Place pl, float* vertices) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= g.nv) return;
    const int m = vmask[v];
    if (!m) return;
    int i, j, k;
    vertex_of(g, v, i, j, k);
    const float sa = sigma[v];
    const float pa[3] = {axis_pos(pl, 0, i), axis_pos(pl, 1, j), axis_pos(pl, 2, k)};
    int64_t out = vscan[v];
    for (int s = 0; s < 7; ++s) {
        if (!((m >> s) & 1)) continue;
        const int bi = i + kOff[s][0], bj = j + kOff[s][1], bk = k + kOff[s][2];
        const float sb = sigma[vid(g, bi, bj, bk)];
        const float t = (level - sa) / (sb - sa);
        const float pb[3] = {axis_pos(pl, 0, bi), axis_pos(pl, 1, bj), axis_pos(pl, 2, bk)};
        if ((uint64_t)out < (uint64_t)max_vertices) {
#pragma unroll
            for (int a = 0; a < 3; ++a) vertices[out * 3 + a] = pa[a] + t * (pb[a] - pa[a]);
        }
        ++out;
    }
}

// output vertex index of the grid edge leaving vertex u along offset s
__device__ __forceinline__ int32_t edge_vertex(const uint8_t* vmask, const int32_t* vscan, int64_t u, int s) {
    return vscan[u] + __popc((unsigned)vmask[u] & ((1u << s) - 1u));
}

__global__ __launch_bounds__(kThreads) void k_mt_emit_faces(Grid g, const float* sigma, float level, const uint8_t* ccnt,
                                                            const int32_t* cscan, const uint8_t* vmask,
                                                            const int32_t* vscan, int64_t max_faces, int32_t* faces) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= g.nc || ccnt[c] == 0) return;
    int i, j, k;
    cell_of(g, c, i, j, k);
    const int corners = cell_corners(g, sigma, level, i, j, k);
    int64_t out = cscan[c];
    for (int t = 0; t < 6; ++t) {
        const int cs = tet_case(corners, t);
        for (int q = 0; q < kTriCount[cs]; ++q) {
            int32_t idx[3];
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                const int te = kTri[cs][q][w];
                int lo[3], hi[3];
                tet_vertex(t, kTetEdge[te][0], lo);
                tet_vertex(t, kTetEdge[te][1], hi);
                const int oi = hi[0] - lo[0], oj = hi[1] - lo[1], ok = hi[2] - lo[2];
                // offset -> edge-id slot: axes 0..2, face diagonals xy 3, xz 4, yz 5, body 6
                const int n = oi + oj + ok;
                const int s = n == 1 ? (oi ? 0 : (oj ? 1 : 2)) : (n == 3 ? 6 : (!ok ? 3 : (!oj ? 4 : 5)));
                idx[w] = edge_vertex(vmask, vscan, vid(g, i + lo[0], j + lo[1], k + lo[2]), s);
            }
            if (kPar[t] < 0) {
                const int32_t x = idx[1];
                idx[1] = idx[2];
                idx[2] = x;
            }
            if ((uint64_t)out < (uint64_t)max_faces) {
#pragma unroll
                for (int w = 0; w < 3; ++w) faces[out * 3 + w] = idx[w];
            }
            ++out;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_grid_points(Grid g, int64_t first, int64_t m, Place pl, float variance,
                                                          float* mean, float* cov) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= m) return;
    int i, j, k;
    vertex_of(g, first + r, i, j, k);
    mean[r * 3 + 0] = axis_pos(pl, 0, i);
    mean[r * 3 + 1] = axis_pos(pl, 1, j);
    mean[r * 3 + 2] = axis_pos(pl, 2, k);
    cov[r * 3 + 0] = variance;
    cov[r * 3 + 1] = variance;
    cov[r * 3 + 2] = variance;
}

struct Epi {
    int64_t M;
    int nc;
    float density_bias, rgb_padding;
    const float *raw_rgb, *raw_den, *grad_mean;
    float *sigma, *albedo, *rgb, *normal;
};

// the activations of compute_graph (models/pano_mip_nerf.py:235-280) with the renderer's arithmetic (pn_render.hip)
__global__ __launch_bounds__(kThreads) void k_field_epilogue(Epi a) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= a.M) return;
    const float* rd = a.raw_den + r * a.nc;
    if (a.sigma) a.sigma[r] = softplus_f(rd[0] + a.density_bias);
    if (a.albedo)
        for (int c = 0; c < 3; ++c) a.albedo[r * 3 + c] = sigmoid_f(rd[1 + c]) * 0.77f + 0.03f;
    if (a.rgb) {
        const float s = 1.f + 2.f * a.rgb_padding;
        for (int c = 0; c < 3; ++c) a.rgb[r * 3 + c] = softplus_f(a.raw_rgb[r * 3 + c]) * s - a.rgb_padding;
    }
    if (a.normal) {
        const float g0 = a.grad_mean[r * 3], g1 = a.grad_mean[r * 3 + 1], g2 = a.grad_mean[r * 3 + 2];
        const float len = fmaxf(sqrtf(g0 * g0 + g1 * g1 + g2 * g2), 1e-12f);
        a.normal[r * 3 + 0] = -g0 / len;
        a.normal[r * 3 + 1] = -g1 / len;
        a.normal[r * 3 + 2] = -g2 / len;
    }
}

// vertex grid of a volume: every axis >= 2 and fewer than 2^31 vertices
int make_grid(int nx, int ny, int nz, Grid& g) {
    if (nx < 2 || ny < 2 || nz < 2) return PN_ERR_BAD_SHAPE;
    g.nx = nx, g.ny = ny, g.nz = nz;
    g.nv = (int64_t)nx * ny * nz;
    g.nc = (int64_t)(nx - 1) * (ny - 1) * (nz - 1);
    return g.nv < ((int64_t)1 << 31) ? PN_OK : PN_ERR_BAD_SHAPE;
}

struct MtWork {
    int64_t vmask, ccnt, vscan, cscan, vblk, cblk, bytes;  // byte offsets
    unsigned nbv, nbc;
};

MtWork mt_work(const Grid& g) {
    MtWork w;
    w.nbv = nblk(g.nv, kItems);
    w.nbc = nblk(g.nc, kItems);
    int64_t o = 0;
    w.vmask = o, o += align256(g.nv);
    w.ccnt = o, o += align256(g.nc);
    w.vscan = o, o += align256(g.nv * 4);
    w.cscan = o, o += align256(g.nc * 4);
    w.vblk = o, o += align256((int64_t)w.nbv * 8);
    w.cblk = o, o += align256((int64_t)w.nbc * 8);
    w.bytes = o;
    return w;
}

Place make_place(float x0, float y0, float z0, float dx, float dy, float dz) {
    Place p;
    p.o[0] = x0, p.o[1] = y0, p.o[2] = z0;
    p.d[0] = dx, p.d[1] = dy, p.d[2] = dz;
    return p;
}

}  // namespace

int pn_grid_points(int nx, int ny, int nz, int64_t first, int64_t m, float x0, float y0, float z0, float dx, float dy,
                   float dz, float variance, float* mean, float* cov, void* stream) {
    Grid g;
    if (make_grid(nx, ny, nz, g) != PN_OK || first < 0 || m < 0 || first > g.nv - m) return PN_ERR_BAD_SHAPE;
    if (m == 0) return PN_OK;
    if (!mean || !cov) return PN_ERR_NULL;
    hipLaunchKernelGGL(k_grid_points, dim3(nblk(m, kThreads)), dim3(kThreads), 0, ST(stream), g, first, m,
                       make_place(x0, y0, z0, dx, dy, dz), variance, mean, cov);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_field_epilogue(int64_t M, int nc, float density_bias, float rgb_padding, const float* raw_rgb,
                      const float* raw_density, const float* grad_mean, float* sigma, float* albedo, float* rgb,
                      float* normal, void* stream) {
    if (M < 0) return PN_ERR_BAD_SHAPE;
    if (nc != 1 && nc != 5) return PN_ERR_UNSUPPORTED;
    if (albedo && nc != 5) return PN_ERR_UNSUPPORTED;
    if (((sigma || albedo) && !raw_density) || (rgb && !raw_rgb) || (normal && !grad_mean)) return PN_ERR_NULL;
    if (M == 0) return PN_OK;
    Epi a{M, nc, density_bias, rgb_padding, raw_rgb, raw_density, grad_mean, sigma, albedo, rgb, normal};
    hipLaunchKernelGGL(k_field_epilogue, dim3(nblk(M, kThreads)), dim3(kThreads), 0, ST(stream), a);
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int64_t pn_mt_work_bytes(int nx, int ny, int nz) {
    Grid g;
    if (make_grid(nx, ny, nz, g) != PN_OK) return PN_ERR_BAD_SHAPE;
    return mt_work(g).bytes;
}

int pn_mt_count(int nx, int ny, int nz, const float* sigma, float level, void* work, int64_t* totals, void* stream) {
    Grid g;
    if (make_grid(nx, ny, nz, g) != PN_OK) return PN_ERR_BAD_SHAPE;
    if (!sigma || !work || !totals) return PN_ERR_NULL;
    const MtWork w = mt_work(g);
    char* base = (char*)work;
    uint8_t *vmask = (uint8_t*)(base + w.vmask), *ccnt = (uint8_t*)(base + w.ccnt);
    int64_t *vblk = (int64_t*)(base + w.vblk), *cblk = (int64_t*)(base + w.cblk);
    hipLaunchKernelGGL(k_mt_classify, dim3(w.nbv + w.nbc), dim3(kThreads), 0, ST(stream), g, sigma, level, w.nbv, vmask,
                       ccnt, vblk, cblk);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mt_scan_blocks, dim3(2), dim3(kScanThreads), 0, ST(stream), vblk, (int64_t)w.nbv, cblk,
                       (int64_t)w.nbc, totals);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mt_fixup, dim3(w.nbv + w.nbc), dim3(kThreads), 0, ST(stream), g, w.nbv, vmask, ccnt, vblk, cblk,
                       (int32_t*)(base + w.vscan), (int32_t*)(base + w.cscan));
    PN_CHECK_LAUNCH();
    return PN_OK;
}

int pn_mt_emit(int nx, int ny, int nz, const float* sigma, float level, const void* work, int64_t num_vertices,
               int64_t num_faces, float x0, float y0, float z0, float dx, float dy, float dz, float* vertices,
               int32_t* faces, void* stream) {
    Grid g;
    if (make_grid(nx, ny, nz, g) != PN_OK) return PN_ERR_BAD_SHAPE;
    const int64_t lim = ((int64_t)1 << 31) - 1;
    if (num_vertices < 0 || num_faces < 0 || num_vertices > lim || num_faces > lim) return PN_ERR_BAD_SHAPE;
    if (!sigma || !work || (num_vertices && !vertices) || (num_faces && !faces)) return PN_ERR_NULL;
    const MtWork w = mt_work(g);
    const char* base = (const char*)work;
    const uint8_t *vmask = (const uint8_t*)(base + w.vmask), *ccnt = (const uint8_t*)(base + w.ccnt);
    const int32_t *vscan = (const int32_t*)(base + w.vscan), *cscan = (const int32_t*)(base + w.cscan);
    if (num_vertices) {
        hipLaunchKernelGGL(k_mt_emit_vertices, dim3(nblk(g.nv, kThreads)), dim3(kThreads), 0, ST(stream), g, sigma,
                           level, vmask, vscan, num_vertices, make_place(x0, y0, z0, dx, dy, dz), vertices);
        PN_CHECK_LAUNCH();
    }
    if (num_faces) {
        hipLaunchKernelGGL(k_mt_emit_faces, dim3(nblk(g.nc, kThreads)), dim3(kThreads), 0, ST(stream), g, sigma, level,
                           ccnt, cscan, vmask, vscan, num_faces, faces);
        PN_CHECK_LAUNCH();
    }
    return PN_OK;
}
