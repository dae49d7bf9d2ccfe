// pn_wgrad.hip - the weight and bias gradients of the radiance MLP: TN GEMMs over the T tensors that the chain kernels
// (pn_chain.hip) left behind, per-workgroup slabs, and their reduction into the flat gradient block.  pn_chain.h holds what the
// two files share (T-tensor element types, the fp16-pair split, the Q24 format, the table of tensor maxima, launch state).
#include "pn_chain.h"

#ifdef PN_TRACE_WG  // debug build only (-DPN_TRACE_WG): shader-clock stamps
__device__ unsigned long long g_chain_trace[64];
extern "C" int pn_chain_trace_read(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chain_trace), sizeof(unsigned long long) * 64) == hipSuccess ? 0 : -4;
}
#endif

// ------------------------------------------------------------------------------------- weight gradients (TN GEMM)
// dW[N1 x N2] (+)= sum over samples X[s][i] * Y[s][j] with X, Y in the T layout (sample-minor), on the bf16 matrix
// cores: A = X^T (k = sample), B = Y.  A workgroup owns the whole [TMW x TNW] result for a contiguous range of
// 16-sample half blocks (split over samples; per-workgroup slabs are reduced afterwards).  Staging: fp32 from HBM to
// registers (full 64-B half rows, coalesced), split ONCE per element into NP bf16 planes, 8-B LDS writes into
// [plane][feature][16 samples] images (the two 16-B pieces of a row swapped on features with bit 3 set: conflict-free
// for the writes and for the ds_read_b128 fragment reads); two LDS buffers, one barrier per half block.  Row sums of X
// (bias gradients) are accumulated from the fp32 values on the way in.
// (Tried: one 256 x 352 tile for layer 5 over [h4 | enc] and one 288 x 256 tile for [extra ; density] over h7, so that
// delta_5 and h7 are read once - 12 accumulator tiles per wave at two waves per SIMD spill 180-280 bytes per lane and the
// weight gradients of an evaluation took 7.2 ms instead of 5.0: the re-reads, 3 GB per step, stay.
// Also tried on the 256 x 256 tile (4.85 ms per evaluation as it stands): staging half block h + 1 piecewise between the
// matrix products of half block h instead of in its own phase in front of the barrier (5.10 ms: the issue port is shared,
// the loads go out later); refilling each piece's registers as soon as it is converted (6.3 ms: the waits degrade to
// vmcnt(0)); four register sets in flight instead of three (4.88 ms: depth is not the limit).  In fact hipcc drains the
// prefetched sets in front of every staging phase (vmcnt(3), (2), (1), (0): it cannot count the younger loads behind the
// conditional `load`); a condition-free steady-state loop with a conditional tail gets vmcnt(13)..(10) - and runs 4.67 ms
// against 4.57 (two sets; three spill): the loop is bound by its conversion + product instruction time, not by latency.
// Round 3: the second half of the waves ONE barrier interval behind the first (same code, three LDS buffers, so that on every
// SIMD one wave stages while its partner multiplies): 6.0-6.2 ms against 4.5 (5.3 with s_setprio around the products) - with
// one multiplying wave per SIMD nothing covers the fragment-read latency at the head of every interval; a barrier that
// waits for LDS traffic only (not vmcnt) in the loop as it stands: no change (profiles/r03_experiments.txt).)
struct WSeg {
    const float* X;  // feature 0 of the X sub-range in block 0
    const float* Y;
    int64_t nhalf;   // 16-sample half blocks
    int FX, FY;      // features per block of the tensors X / Y live in
    int bias;        // rows of this segment count towards the row sums of X (the second-order rows do not)
    const uint32_t* ax;  // NP = 2: largest |x| of the whole X / Y tensor (float bits, written by the chain kernels): the
    const uint32_t* ay;  // segment's operands are scaled by ONE power of two each (the sum runs over all samples)
};
struct WgArgs {
    WSeg seg[4];
    int nseg;
    int64_t half_total, per;
    float* slab;
    int64_t slab_stride;
    int bias;
};
// ONE launch runs up to WG_MAXJ jobs of the same tile configuration and operand format (grid.y = job): the six 256 x 256 trunk
// layers whose operands are both Q24, or layer 0 and the skip columns of layer 5.  Every job gets 1 / n of the CUs and n times the
// sample range per workgroup: the same parallelism with 1 / n of the launches, of the slab bytes (a workgroup writes its 257 KB of
// partial sums once per n times as many half blocks) and of the slab reductions - a job costs ~40 us whatever its size (prologue,
// slab write, reduction launch), 18 % of the 512-ray step in fifteen separate launches.
constexpr int WG_MAXJ = 8;
struct WgMulti {
    WgArgs job[WG_MAXJ];
};

template <int NP>
__device__ __forceinline__ f32x16 mfma_split32(const BFrag<NP>& a, const BFrag<NP>& b, f32x16 v) {
    if constexpr (NP == 3) {  // small terms first
        v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[2], b.p[0], v, 0, 0, 0);
        v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[0], b.p[2], v, 0, 0, 0);
        v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[1], b.p[1], v, 0, 0, 0);
        v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[1], b.p[0], v, 0, 0, 0);
        v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[0], b.p[1], v, 0, 0, 0);
        v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[0], b.p[0], v, 0, 0, 0);
    } else if constexpr (NP == 2) {
        v = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.p[1], b.p[0], v, 0, 0, 0);
        v = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.p[0], b.p[1], v, 0, 0, 0);
        v = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.p[0], b.p[0], v, 0, 0, 0);
    } else {
        v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[0], b.p[0], v, 0, 0, 0);
    }
    return v;
}
// the T tensors are read once per GEMM: non-temporal loads (4.70 -> 4.57 ms for the GEMMs of one evaluation)
#define WG_LD(p) __builtin_nontemporal_load(p)
// The three 16-byte loads of a Q24 unit (48 bytes, stride 48 across the lanes): each instruction touches a third of every 128-byte
// line of the wave's 3 KB.  As NON-temporal loads each of the three fetched its lines from L2 on its own - TCP_TCC_READ_REQ 7.63e7 per
// launch of the 256 x 256 tile against 2.57e7 TCC_EA0_RDREQ, two L2 hits per miss; as plain loads the second and third hit the lines
// the first brought into the vector L1: 2.52e7 requests, no L2 hits (profiles/r04_wgrad_unit_loads.txt).  The kernel itself is no
// faster (761 us under the counters either way: it is not bound by L2 requests), the training step 0.65 % (same box, twice).
// Y24 / X24: the operand tensor is stored in Q24 (see pack_q24): its work item is a UNIT of 48 contiguous bytes - four features of
// four samples - unpacked to fp32 (one byte permute per element) and transposed in registers into four (feature, 4 samples) pieces.
// With both operands in Q24 the X and Y units form one list over the threads (one unit per thread on the 256 x 256 tile).  The LDS
// image then holds feature f in row (f & ~3) | ((f + (f >> 2)) & 3): a unit's four writes go to rows 4 qb + f for a fixed f across
// the wave, which in the plain image are 128 bytes apart - the same eight banks sixteen times.
template <int NP, int TM, int TN, int WM, int WN, bool X24 = false, bool Y24 = false>
__global__ __launch_bounds__(64 * WM * WN) void k_chain_wgrad(WgMulti multi) {
    const WgArgs& a = multi.job[blockIdx.y];
    static_assert(!(X24 || Y24) || NP == 2, "Q24 tensors exist with fp16 pairs only");
    static_assert(!X24 || Y24, "combinations in use: (0,0), (0,1), (1,1)");
    constexpr bool ROT = X24 || Y24;  // row permutation of the LDS images
    constexpr int NTH = 64 * WM * WN, TMW = 32 * TM * WM, TNW = 32 * TN * WN;
    constexpr int PX = TMW * 16, PY = TNW * 16;     // bf16 elements per plane
    constexpr int BUF = NP * (PX + PY);             // per buffer
    typedef typename TEl<NP>::type TE;              // element type of the T tensors (bf16 for NP = 1: staging is a copy)
    constexpr int PPR = 16 * (int)sizeof(TE) / 16;  // 16-B pieces per row of 16 samples: 4 (fp32) or 2 (bf16)
    constexpr int SPP = 16 / PPR;                   // samples per piece
    constexpr int CX = X24 ? 0 : TMW * PPR, CY = Y24 ? 0 : TNW * PPR;   // 16-B pieces per half block (fp32 / bf16 operands)
    constexpr int LX = X24 ? 1 : (CX + NTH - 1) / NTH, LY = Y24 ? 1 : (CY + NTH - 1) / NTH;  // (1: a dummy register)
    constexpr int UX = X24 ? TMW : 0, UY = Y24 ? TNW : 0;               // Q24 units per half block
    constexpr int LU = (UX + UY + NTH - 1) / NTH;                       // units per thread (X units first, then Y units)
    static_assert(UX % 64 == 0, "a wave's units are all X or all Y");
    // Q24 units: a lane loads its unit as three 16-byte pieces of its own - lanes 48 bytes apart, every instruction touching a third
    // of each of 24 lines.  That streamed at 2.8 TB/s with nothing else in the kernel (timing ablations,
    // profiles/r04_wgrad_timing_ablations.txt: 570 us for 1.61 GB, the same with or without staging and barriers, 824 us for the
    // whole kernel), against 5.8 - 6.0 TB/s for the tiles whose loads are contiguous across the lanes.  (Tried and dropped: three
    // fully coalesced 1-KB loads per wave, turned into units through a wave-private 3-KB scratch in LDS.)
    __shared__ __attribute__((aligned(16))) unsigned short smem[2 * BUF];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid / WN, wn = wid % WN;
    const int64_t h0 = (int64_t)blockIdx.x * a.per;
    if (h0 >= a.half_total) return;  // (uniform: a job of a multi-job launch with fewer workgroups than grid.x; no slab of its own)
    int64_t h1 = h0 + a.per;
    if (h1 > a.half_total) h1 = a.half_total;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    float bsum[LX];
#pragma unroll
    for (int i = 0; i < LX; ++i) bsum[i] = 0.f;
    float bsum4[LU > 0 ? LU : 1][4] = {};  // X24: row sums of a unit's four features

    // NSET register sets: the loads of half block h + NSET are issued when h's set has been staged, so they have NSET
    // half blocks to land (one workgroup per CU: nothing else hides the HBM latency).  Three where the registers allow:
    // with three products per fp32 product the kernel is HBM-bound and two sets keep only 32-64 KB per CU in flight.
    // (both operands in Q24: a thread holds ONE 48-byte unit per set - four sets are the 48 registers of three fp32 sets)
    constexpr int NSET = (X24 && LU == 1) ? 4 : ((NP <= 2 && (X24 ? 0 : LX) + (Y24 ? 0 : LY) + 3 * LU <= 4) ? 3 : 2);
    f32x4 xr[NSET][LX], yr[NSET][LY];
    f32x4 ur[NSET][LU > 0 ? LU : 1][3];  // a unit: 48 bytes
    // the 256 x 256 tile on Q24 operands (one or both) and on bf16 tensors: measured same box, us per launch in the training step,
    // common -> alternating order: both in Q24 821 -> 783, Y in Q24 892 -> 832, bf16 tensors 426 -> 358; NOT on fp32 tensors with
    // fp16 pairs (589 -> 644) or the six-product split (1230 -> 1258)
    constexpr bool ALT = (WM * WN == 8 && TM == 2 && TN == 4) && (X24 || Y24 || NP == 1);  // (see the loop)
    // (Measured and dropped in the alternating loop: the two halves of the workgroup swapping the X units - whose row sums cost a
    // wave ~500 cycles more per half block - with the parity of the half block: 828 us per launch with or without.)
    auto unit_of = [&](int i) { return tid + NTH * i; };
    float bw[NSET] = {};  // bias weight of the half block held in each set
    // NP = 2: ONE unit for the whole job, 2^unit = the scale of every product in the accumulators: the smallest sx + sy over
    // the job's segments (the segment with the LARGEST products).  A segment whose own exponents add up to more is scaled
    // down by the difference (its products are that many binades below the dominant segment's; what falls below fp16's
    // range there is below 2^-39 of the dominant products) - no accumulator is ever re-based, so sums cannot overflow
    // however far the segments' magnitudes are apart, and the result does not depend on where a workgroup's range starts.
    int sx[NSET] = {}, sy[NSET] = {}, unit = 0;
    auto seg_exps = [&](const WSeg& S, int& ex, int& ey) {
        ex = scale_exp(__uint_as_float(*S.ax), EXP_CAP_Z);
        ey = scale_exp(__uint_as_float(*S.ay), EXP_CAP_Z);
        int over = ex + ey - unit;                      // >= 0
        const int rx = over < ex + 126 ? over : ex + 126;  // pow2f takes -126 .. 127
        ex -= rx;
        ey -= over - rx;
        if (ey < -126) ey = -126;                       // (everything of the segment has long been flushed to zero)
    };
    if constexpr (NP == 2) {
        unit = 1 << 20;
        for (int i = 0; i < a.nseg; ++i) {
            const int e = scale_exp(__uint_as_float(*a.seg[i].ax), EXP_CAP_Z) + scale_exp(__uint_as_float(*a.seg[i].ay), EXP_CAP_Z);
            unit = e < unit ? e : unit;
        }
    }
    // Segment cursor of the loads (half blocks are loaded in increasing order): the segment's pointers, widths and
    // exponents are fetched when the range crosses into it, not per half block - two dependent scalar loads in front of
    // every half block's global loads otherwise.
    // (Do NOT force the cursor into scalar registers with v_readfirstlane: hipcc then waits s_waitcnt vmcnt(0) - for every operand
    // load in flight - in front of every staging instead of the counted vmcnt(9) / (11) of the alternating loop; as written the
    // segment's fields come by scalar loads and only the segment switch, which reads the two tensor maxima, drains.)
    int csg = 0, cFX = a.seg[0].FX, cFY = a.seg[0].FY, csx = 0, csy = 0;
    int64_t cbase = 0, cend = a.seg[0].nhalf;
    const TE* cX = reinterpret_cast<const TE*>(a.seg[0].X);
    const TE* cY = reinterpret_cast<const TE*>(a.seg[0].Y);
    float cbw = a.seg[0].bias ? 1.f : 0.f;
    if constexpr (NP == 2) seg_exps(a.seg[0], csx, csy);
    auto load = [&](int64_t h, int set) __attribute__((always_inline)) {
        while (csg + 1 < a.nseg && h >= cend) {  // (uniform; the last segment takes what is left)
            ++csg;
            const WSeg& S = a.seg[csg];
            cbase = cend;
            cend += S.nhalf;
            cX = reinterpret_cast<const TE*>(S.X);
            cY = reinterpret_cast<const TE*>(S.Y);
            cFX = S.FX;
            cFY = S.FY;
            cbw = S.bias ? 1.f : 0.f;
            if constexpr (NP == 2) seg_exps(S, csx, csy);
        }
        const int64_t hb = h - cbase;
        bw[set] = cbw;
        if constexpr (NP == 2) {
            sx[set] = csx;
            sy[set] = csy;
        }
        const int64_t blk = hb;  // a T-layout sample block is one half block
        const TE* xb = cX + blk * ((int64_t)cFX * TILE);
        const TE* yb = cY + blk * ((int64_t)cFY * TILE);
        if constexpr (!X24) {
#pragma unroll
            for (int i = 0; i < LX; ++i) {
                const int idx = tid + NTH * i;
                if (CX % NTH == 0 || idx < CX) xr[set][i] = WG_LD(reinterpret_cast<const f32x4*>(xb + (idx / PPR) * TILE + (idx % PPR) * SPP));
            }
        }
        if constexpr (!Y24) {
#pragma unroll
            for (int i = 0; i < LY; ++i) {
                const int idx = tid + NTH * i;
                if (CY % NTH == 0 || idx < CY) yr[set][i] = WG_LD(reinterpret_cast<const f32x4*>(yb + (idx / PPR) * TILE + (idx % PPR) * SPP));
            }
        }
        if constexpr (X24 || Y24) {  // (a Q24 block of F features is F * 48 bytes, a unit 48)
            const unsigned char* xq = reinterpret_cast<const unsigned char*>(cX) + blk * ((int64_t)cFX * 48);
            const unsigned char* yq = reinterpret_cast<const unsigned char*>(cY) + blk * ((int64_t)cFY * 48);
#pragma unroll
            for (int i = 0; i < LU; ++i) {
                const int u = unit_of(i);
                if ((UX + UY) % NTH == 0 || u < UX + UY) {
                    const f32x4* p = reinterpret_cast<const f32x4*>(u < UX ? xq + u * 48 : yq + (u - UX) * 48);  // (wave-uniform)
                    ur[set][i][0] = p[0];  // (plain loads: see above)
                    ur[set][i][1] = p[1];
                    ur[set][i][2] = p[2];
                }
            }
        }
    };
    auto put = [&](unsigned short* plane0, int pstride, int idx, const f32x4& v, int ex) {
        if constexpr (NP == 1) {  // the piece already holds 8 bf16 samples of one feature: copy
            const int f = idx >> 1, q = idx & 1;
            *reinterpret_cast<f32x4*>(plane0 + f * 16 + ((q ^ ((f >> 3) & 1)) << 3)) = v;
            return;
        }
        const int f0 = idx >> 2, q = idx & 3;
        const int f = ROT ? ((f0 & ~3) | ((f0 + (f0 >> 2)) & 3)) : f0;
        const int o = f * 16 + (((q >> 1) ^ ((f >> 3) & 1)) << 3) + (q & 1) * 4;
        if constexpr (NP == 2) {
            const float s = pow2f(ex);
            const float x4[4] = {v[0], v[1], v[2], v[3]};
            uint32_t h2[2], l2[2];
            split2_pairs<2>(x4, s, h2, l2);
            *reinterpret_cast<uint2*>(plane0 + o) = make_uint2(h2[0], h2[1]);
            *reinterpret_cast<uint2*>(plane0 + pstride + o) = make_uint2(l2[0], l2[1]);
        } else {
            typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
            bf16x4 hv, mv, lv;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const __bf16 hb = (__bf16)v[c];
                hv[c] = hb;
                if constexpr (NP == 3) {
                    const float r1 = v[c] - (float)hb;
                    const __bf16 mb = (__bf16)r1;
                    mv[c] = mb;
                    lv[c] = (__bf16)(r1 - (float)mb);
                }
            }
            *reinterpret_cast<bf16x4*>(plane0 + o) = hv;
            if constexpr (NP == 3) {
                *reinterpret_cast<bf16x4*>(plane0 + pstride + o) = mv;
                *reinterpret_cast<bf16x4*>(plane0 + 2 * pstride + o) = lv;
            }
        }
    };
    // a Q24 unit -> four (feature, 4 samples) pieces of the image at `plane0`; `bs`: the unit's row sums (X with bias) or null
    auto put_unit = [&](unsigned short* plane0, int pstride, int u, const f32x4 (&r)[3], int ex, float* bs, float w) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        uint32_t d[12];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u32x4 t = __builtin_bit_cast(u32x4, r[k]);
#pragma unroll
            for (int c = 0; c < 4; ++c) d[4 * k + c] = t[c];
        }
        float e[4][4];  // [sample][feature]
#pragma unroll
        for (int sm = 0; sm < 4; ++sm) {
            e[sm][0] = __uint_as_float(d[3 * sm] << 8);
            e[sm][1] = __uint_as_float(__builtin_amdgcn_perm(d[3 * sm + 1], d[3 * sm], 0x0504030cu));
            e[sm][2] = __uint_as_float(__builtin_amdgcn_perm(d[3 * sm + 2], d[3 * sm + 1], 0x0403020cu));
            e[sm][3] = __uint_as_float(d[3 * sm + 2] & 0xffffff00u);
        }
        const int qb = u >> 2, sg = u & 3;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const f32x4 v{e[0][f], e[1][f], e[2][f], e[3][f]};
            put(plane0, pstride, (4 * qb + f) * 4 + sg, v, ex);
            if (bs) bs[f] += w * ((v[0] + v[1]) + (v[2] + v[3]));
        }
    };
    auto stage = [&](int buf, int set) __attribute__((always_inline)) {
        unsigned short* xs = smem + buf * BUF;
        unsigned short* ys = xs + NP * PX;
        if constexpr (PN_ABL_WG & 2) {  // keep the loads alive, convert nothing
            if constexpr (X24 || Y24) {
#pragma unroll
                for (int i = 0; i < LU; ++i) asm volatile("" ::"v"(ur[set][i][0]), "v"(ur[set][i][1]), "v"(ur[set][i][2]));
            }
            if constexpr (!X24) {
#pragma unroll
                for (int i = 0; i < LX; ++i) asm volatile("" ::"v"(xr[set][i]));
            }
            if constexpr (!Y24) {
#pragma unroll
                for (int i = 0; i < LY; ++i) asm volatile("" ::"v"(yr[set][i]));
            }
            return;
        }
        if constexpr (X24 || Y24) {
#pragma unroll
            for (int i = 0; i < LU; ++i) {
                const int u = unit_of(i);
                if ((UX + UY) % NTH == 0 || u < UX + UY) {
                    if (u < UX) put_unit(xs, PX, u, ur[set][i], sx[set], bsum4[i], bw[set]);  // (wave-uniform)
                    else put_unit(ys, PY, u - UX, ur[set][i], sy[set], nullptr, 0.f);
                }
            }
        }
        if constexpr (!X24)
#pragma unroll
        for (int i = 0; i < LX; ++i) {
            const int idx = tid + NTH * i;
            if (CX % NTH == 0 || idx < CX) {
                put(xs, PX, idx, xr[set][i], sx[set]);
                if constexpr (NP == 1) {
                    const bf16x8 hv = __builtin_bit_cast(bf16x8, xr[set][i]);
                    float t = 0.f;
#pragma unroll
                    for (int c = 0; c < 8; ++c) t += (float)hv[c];
                    bsum[i] += bw[set] * t;
                } else {
                    bsum[i] += bw[set] * ((xr[set][i][0] + xr[set][i][1]) + (xr[set][i][2] + xr[set][i][3]));
                }
            }
        }
        if constexpr (!Y24)
#pragma unroll
        for (int i = 0; i < LY; ++i) {
            const int idx = tid + NTH * i;
            if (CY % NTH == 0 || idx < CY) put(ys, PY, idx, yr[set][i], sy[set]);
        }
    };
    const int fr = lane & 31, fh = lane >> 5;
    auto frag = [&](const unsigned short* plane, int feature) {
        if constexpr (ROT) feature = (feature & ~3) | ((feature + (feature >> 2)) & 3);
        return *reinterpret_cast<const typename PlaneOf<NP>::type*>(plane + feature * 16 + ((fh ^ ((feature >> 3) & 1)) << 3));
    };
    auto compute = [&](int buf) __attribute__((always_inline)) {
        if constexpr (PN_ABL_WG & 1) return;
        const unsigned short* xs = smem + buf * BUF;
        const unsigned short* ys = xs + NP * PX;
        // The Y fragments of tile column j + 1 are read BEFORE the products of column j, by inline asm with hand-counted waits.  As one
        // fragment set re-used per column (round 3) every column's products waited for an LDS round trip with the matrix pipe idle -
        // four bubbles of 150 - 200 cycles in a wave's 768 cycles of products per half block, in the phase in which its SIMD partner
        // is staging and cannot fill them: the 256 x 256 tile ran 3300 cycles per half block against 1536 of matrix pipe, with its
        // loads long landed (timing ablations: the loads alone stream at 5.7 TB/s, the kernel moved 3.9:
        // profiles/r04_wgrad_timing_ablations.txt).  Written as plain C++ with two fragment sets hipcc still allocates ONE and
        // issues each read behind the last product that uses the old value, one instruction in front of its wait.
        // NOT on the tile with both operands in Q24: its four register sets of units leave no room for a second fragment set
        // (12 registers spilled: 950 us per launch against 739; with three sets 744 - no gain either way: that tile's critical
        // path is the staging of its X units, section 14 of profiles/r03_experiments.txt).  Measured on the others, same box, us
        // per launch in the training step: fp32 tensors 596 -> 545, Y in Q24 788 -> 752 (profiles/r04_wgrad_fragment_prefetch.txt).
        if constexpr (X24) {
            BFrag<NP> af[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int p = 0; p < NP; ++p) af[i].p[p] = frag(xs + p * PX, 32 * (wm * TM + i) + fr);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                BFrag<NP> bf;
#pragma unroll
                for (int p = 0; p < NP; ++p) bf.p[p] = frag(ys + p * PY, 32 * (wn * TN + j) + fr);
#pragma unroll
                for (int i = 0; i < TM; ++i) acc[i][j] = mfma_split32<NP>(af[i], bf, acc[i][j]);
            }
            return;
        }
        typedef typename PlaneOf<NP>::type Frag;
        auto lds_of = [](const unsigned short* q) { return (uint32_t)(uintptr_t)(lds_ptr_t)q; };
        auto fidx = [&](int feature) {  // element index of this lane's fragment of `feature` in a plane (see frag)
            if constexpr (ROT) feature = (feature & ~3) | ((feature + (feature >> 2)) & 3);
            return feature * 16 + ((fh ^ ((feature >> 3) & 1)) << 3);
        };
        // 32 more features are 512 more elements whatever the lane (the row permutation and the 16-byte swap act on fr alone)
        const uint32_t xa = lds_of(xs) + 2 * fidx(32 * (wm * TM) + fr), ya = lds_of(ys) + 2 * fidx(32 * (wn * TN) + fr);
        // (offsets as immediates: one address register per operand instead of one per read)
        auto rd = [](Frag& dst, uint32_t addr, auto off) {
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(decltype(off)::value) : "memory");
        };
        static_assert(2 * NP * PX + 1024 * TM < 65536 && 2 * NP * PY + 1024 * TN < 65536, "16-bit offset field of ds_read_b128");
        BFrag<NP> af[TM];
        BFrag<NP> bf[2];
        auto read_b = [&](auto jc, BFrag<NP>& f) {  // Y fragments of tile column j
            constexpr int J = decltype(jc)::value;
            static_for<NP>([&](auto pc) {
                constexpr int P = decltype(pc)::value;
                rd(f.p[P], ya, std::integral_constant<int, 1024 * J + 2 * P * PY>{});
            });
        };
        // all but the newest `left` reads have returned; ties the registers the products read to the wait
        auto settle = [&](auto left, BFrag<NP>& f) {
            constexpr int L = decltype(left)::value;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if (p == 0) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(f.p[p]) : "n"(L) : "memory");
                else asm volatile("" : "+v"(f.p[p]));
            }
        };
        read_b(std::integral_constant<int, 0>{}, bf[0]);
        static_for<TM>([&](auto ic) {
            constexpr int I = decltype(ic)::value;
            static_for<NP>([&](auto pc) {
                constexpr int P = decltype(pc)::value;
                rd(af[I].p[P], xa, std::integral_constant<int, 1024 * I + 2 * P * PX>{});
            });
        });
        if constexpr (TN > 1) {
            read_b(std::integral_constant<int, 1>{}, bf[1]);
            settle(std::integral_constant<int, NP>{}, bf[0]);
        } else {
            settle(std::integral_constant<int, 0>{}, bf[0]);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int p = 0; p < NP; ++p) asm volatile("" : "+v"(af[i].p[p]));
        static_for<TN>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
#pragma unroll
            for (int i = 0; i < TM; ++i) acc[i][J] = mfma_split32<NP>(af[i], bf[J & 1], acc[i][J]);
            if constexpr (J + 2 < TN) {  // column J + 2 into the set column J's products have just been issued from
                __builtin_amdgcn_sched_barrier(0);
                read_b(std::integral_constant<int, J + 2>{}, bf[J & 1]);
            }
            if constexpr (J + 1 < TN) {
                if constexpr (J + 2 < TN) settle(std::integral_constant<int, NP>{}, bf[(J + 1) & 1]);
                else settle(std::integral_constant<int, 0>{}, bf[(J + 1) & 1]);
            }
        });
    };
#ifdef PN_TRACE_WG  // debug build only: phase times of workgroup 0 (every wave), summed over its half blocks
    unsigned long long tw[4] = {0, 0, 0, 0};
#define WGT(i, expr)                                                   \
    do {                                                               \
        const unsigned long long t0_ = __builtin_amdgcn_s_memtime();   \
        expr;                                                          \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             \
        tw[i] += __builtin_amdgcn_s_memtime() - t0_;                   \
    } while (0)
#else
#define WGT(i, expr) expr
#endif
    // half block h + K of a trip: register set K % NSET, LDS buffer K % 2 (static indices)
    auto one = [&](auto kc, int64_t h) __attribute__((always_inline)) {
        constexpr int K = decltype(kc)::value;
        if (h + K < h1) {  // (uniform)
            WGT(0, stage(K % 2, K % NSET));
            WGT(1, __syncthreads());
            WGT(2, if (h + K + NSET < h1) load(h + K + NSET, K % NSET));
            WGT(3, compute(K % 2));
        }
    };
    if constexpr (ALT) {
        // ALTERNATING ORDER.  In the common order (below) both waves of a SIMD stage, then both multiply; the phase trace
        // (tools/experiments/trace_wgrad.py) showed the second-dispatched wave of every SIMD losing the arbitration for the matrix pipe,
        // finishing its products last and only then starting to stage: the pipe idle for half of every half block.  Here wave
        // type t (0: waves 0 .. NW/2 - 1, 1: their SIMD partners) runs   products(K) ; stage(K + 1 + t) ; refill   per half block
        // K - ONE instruction sequence - with its barrier behind the products (t = 1) or behind the staging (t = 0): after a
        // barrier one wave of a SIMD multiplies while its partner converts, then they swap.  The partner is one half block
        // ahead in its staging (it staged half block 1 in the prologue), its LDS buffer index the only run-time difference; the
        // register set of a staging is (K + 1) % NSET for both, the loads are unconditional (past the end: the last half block
        // again, never staged) so that hipcc counts them.  Hazards: a wave stages into buffer b only behind a barrier that
        // everyone passed after its products from b; products from b start behind a barrier everyone passed after staging b.
        const int t = wid >= (WM * WN) / 2 ? 1 : 0;  // (wave-uniform)
        const int64_t n = h1 - h0;
        auto clampd = [&](int64_t hb) { return h0 + (hb < n ? hb : n - 1); };
        if (n > 0) {
            load(h0, 0);
            stage(0, 0);
            load(clampd(1), 0);          // (type 0 does not need it: issued by every wave so that hipcc's count of the loads in
            if (t && 1 < n) stage(1, 0);  //  flight is the same on every path into the loop)
#pragma unroll
            for (int sidx = 1; sidx < NSET; ++sidx) load(clampd(sidx + t), sidx);
            load(clampd(NSET + t), 0);
            __syncthreads();
            constexpr int TRIPA = NSET == 3 ? 6 : (NSET == 4 ? 4 : 2);
            auto alt = [&](auto kc, auto guard, int64_t k0) __attribute__((always_inline)) {
                constexpr int K = decltype(kc)::value;
                if (!decltype(guard)::value || k0 + K < n) {  // (uniform)
                    WGT(3, compute(K % 2));
                    if (t && !(PN_ABL_WG & 4)) WGT(1, __syncthreads());
                    const int64_t hb = k0 + K + 1 + t;
                    if (hb < n) WGT(0, stage((K + 1 + t) & 1, (K + 1) % NSET));
                    WGT(2, load(clampd(hb + NSET), (K + 1) % NSET));
                    if (!t && !(PN_ABL_WG & 4)) WGT(1, __syncthreads());
                }
            };
            int64_t k0 = 0;
            for (; k0 + TRIPA <= n; k0 += TRIPA) {  // whole trips: no condition around a half block (hipcc counts the loads)
                alt(std::integral_constant<int, 0>{}, std::false_type{}, k0);
                alt(std::integral_constant<int, 1>{}, std::false_type{}, k0);
                if constexpr (TRIPA >= 4) {
                    alt(std::integral_constant<int, 2>{}, std::false_type{}, k0);
                    alt(std::integral_constant<int, 3>{}, std::false_type{}, k0);
                }
                if constexpr (TRIPA == 6) {
                    alt(std::integral_constant<int, 4>{}, std::false_type{}, k0);
                    alt(std::integral_constant<int, 5>{}, std::false_type{}, k0);
                }
            }
            if (k0 < n) {  // the last, partial trip
                alt(std::integral_constant<int, 0>{}, std::true_type{}, k0);
                alt(std::integral_constant<int, 1>{}, std::true_type{}, k0);
                if constexpr (TRIPA >= 4) {
                    alt(std::integral_constant<int, 2>{}, std::true_type{}, k0);
                    alt(std::integral_constant<int, 3>{}, std::true_type{}, k0);
                }
                if constexpr (TRIPA == 6) {
                    alt(std::integral_constant<int, 4>{}, std::true_type{}, k0);
                    alt(std::integral_constant<int, 5>{}, std::true_type{}, k0);
                }
            }
        }
    } else
    if (h0 < h1) {
#pragma unroll
        for (int k = 0; k < NSET; ++k)
            if (h0 + k < h1) load(h0 + k, k);
        constexpr int TRIP = NSET == 3 ? 6 : (NSET == 4 ? 4 : 2);  // a multiple of the sets and of the two LDS buffers
        // (The loads stay conditional.  Whole trips without a condition, every half block refilling its set, let hipcc COUNT the loads
        // in flight - vmcnt(9) / (6) where the conditional form drains the prefetched sets, vmcnt(2), (1), (0) - and measured 827 - 831
        // us per launch against 807 in the training step: the waits are not what the half block's time is made of.)
        for (int64_t h = h0; h < h1; h += TRIP) {
            one(std::integral_constant<int, 0>{}, h);
            one(std::integral_constant<int, 1>{}, h);
            if constexpr (TRIP == 4) {
                one(std::integral_constant<int, 2>{}, h);
                one(std::integral_constant<int, 3>{}, h);
            }
            if constexpr (TRIP == 6) {
                one(std::integral_constant<int, 2>{}, h);
                one(std::integral_constant<int, 3>{}, h);
                one(std::integral_constant<int, 4>{}, h);
                one(std::integral_constant<int, 5>{}, h);
            }
        }
    }
#ifdef PN_TRACE_WG
    if (blockIdx.x == 0 && lane == 0 && (X24 && Y24)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) g_chain_trace[8 * i + wid] = tw[i];
        if (wid == 0) g_chain_trace[32] = (unsigned long long)(h1 - h0);
    }
#endif
    float* out = a.slab + (int64_t)blockIdx.x * a.slab_stride;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = 32 * (wm * TM + i) + (e & 3) + 8 * (e >> 2) + 4 * fh;
                const float x = acc[i][j][e];
                out[(int64_t)row * TNW + 32 * (wn * TN + j) + fr] = NP == 2 ? ldexpf(x, -unit) : x;
            }
    if constexpr (X24) {
        if (a.bias) {
#pragma unroll
            for (int i = 0; i < LU; ++i) {
                const int u = tid + NTH * i;
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    float v = bsum4[i][f];
                    v += __shfl_xor(v, 1, 64);
                    v += __shfl_xor(v, 2, 64);
                    if ((u & 3) == 0 && u < UX) out[(int64_t)TMW * TNW + 4 * (u >> 2) + f] = v;
                }
            }
        }
    } else if (a.bias) {
#pragma unroll
        for (int i = 0; i < LX; ++i) {
            float v = bsum[i];
            v += __shfl_xor(v, 1, 64);
            if constexpr (PPR == 4) v += __shfl_xor(v, 2, 64);
            const int idx = tid + NTH * i;
            if (idx % PPR == 0 && (CX % NTH == 0 || idx < CX)) out[(int64_t)TMW * TNW + idx / PPR] = v;
        }
    }
}

// ---- weight gradients of one training step -------------------------------------------------------------------
struct WgJob {
    WSeg seg[4];
    int nseg;
    int cfg;            // 0: 256x256, 1: 256x96, 2: 128x288, 3: 32x256, 4: 32x128
    int rows, cols;     // valid part of the result
    float* dst; int ldd;
    float* dbias;       // or null
    int fmt;            // cfg 0, fp16 pairs: 0 both operands fp32, 1 Y in Q24, 3 X and Y in Q24 (see pack_q24)
};
static const int kCfgM[5] = {256, 256, 128, 32, 32};
static const int kCfgN[5] = {256, 96, 288, 256, 128};

// Slab reduction of the jobs of one launch (grid.y = job): dst[r][c] += sum over the job's nb slabs of their [rows x cols] part
// (leading dimension src_ld), and dbias[i] += sum of the slabs' row sums (at slab offset bias_off), in a fixed order (64 elements per
// workgroup, four partial sums each, eight loads in flight): 31 reduction launches per training step were 16 % of its launches at
// the 512-ray share.
struct RedJob {
    const float* slabs;
    int64_t nb, stride, bias_off;
    int rows, cols, src_ld, ldd;
    float* dst;
    float* dbias;
};
constexpr int RED_MAXJ = WG_MAXJ;
struct RedMulti {
    RedJob job[RED_MAXJ];
};
__global__ __launch_bounds__(256) void k_reduce_job(RedMulti multi) {
    const RedJob& J = multi.job[blockIdx.y];
    const float* slabs = J.slabs;
    const int64_t nb = J.nb, stride = J.stride;
    const int rows = J.rows, cols = J.cols;
    float* dbias = J.dbias;
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + tx, nw = rows * cols, n = nw + (dbias ? rows : 0);
    if (blockIdx.x * 64 >= n) return;  // (uniform: a smaller job of the launch)
    float acc = 0.f;
    float* d = nullptr;
    if (e < n) {
        const float* p;
        if (e < nw) {
            const int r = e / cols, c = e - r * cols;
            p = slabs + (int64_t)r * J.src_ld + c;
            d = J.dst + (int64_t)r * J.ldd + c;
        } else {
            p = slabs + J.bias_off + (e - nw);
            d = dbias + (e - nw);
        }
        int64_t b = ty;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f;
        for (; b + 28 < nb; b += 32) {
            a0 += p[b * stride];
            a1 += p[(b + 4) * stride];
            a2 += p[(b + 8) * stride];
            a3 += p[(b + 12) * stride];
            a4 += p[(b + 16) * stride];
            a5 += p[(b + 20) * stride];
            a6 += p[(b + 24) * stride];
            a7 += p[(b + 28) * stride];
        }
        for (; b < nb; b += 4) a0 += p[b * stride];
        acc = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
    }
    red[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && e < n) *d += (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}

// jobs [j0, j0 + nj) of `jobs`: same tile configuration and operand format, disjoint destinations -> one GEMM launch + one reduction
static int run_reduce(const std::vector<RedJob>& red, size_t i0, size_t i1, hipStream_t s);
// (One reduction launch per group, the workspace reused by the next group.  Keeping every group's slabs until ONE reduction launch
// at the end of the step - thirteen launches fewer, 0.9 GB of workspace - measured no gain, eager or replayed:
// profiles/r04_launch_merge_ab.txt.)
template <int NP>
static int run_wgrad_group(const WgJob* jobs, int nj, float* work, int64_t work_floats, int max_wgs, hipStream_t s) {
    int64_t used = 0;
    std::vector<RedJob> red;
    if (nj < 1 || nj > WG_MAXJ) return PN_ERR_BAD_SHAPE;
    const WgJob& j0 = jobs[0];
    const int TMW = kCfgM[j0.cfg], TNW = kCfgN[j0.cfg];
    const int64_t stride = (int64_t)TMW * TNW + TMW;
    // workgroups per CU the configuration's registers and LDS allow (the narrow tiles: 146 / 100 registers per lane,
    // 37 / 20 KB): more sample ranges in flight, their staging and product phases interleave
    static const int kPerCu[5] = {1, 1, 1, 3, 4};
    int cus = chain_cus();
    if (max_wgs > 0 && max_wgs < cus) cus = max_wgs;  // the CUs this launch may occupy (the rest run a chain kernel of another stream)
    const int64_t slots = (int64_t)cus * kPerCu[j0.cfg] / nj;  // workgroups per job
    WgMulti m{};
    int64_t nsplit_max = 0, slab0 = 0;
    float* const base = work + used;
    double flops = 0;
    for (int q = 0; q < nj; ++q) {
        const WgJob& j = jobs[q];
        if (j.cfg != j0.cfg || j.fmt != j0.fmt) return PN_ERR_BAD_SHAPE;
        WgArgs& a = m.job[q];
        int64_t total = 0;
        for (int i = 0; i < j.nseg; ++i) {
            a.seg[i] = j.seg[i];
            total += j.seg[i].nhalf;
        }
        a.nseg = j.nseg;
        a.half_total = total;
        int64_t nsplit = slots < 1 ? 1 : slots;
        if (nsplit > (total + 3) / 4) nsplit = (total + 3) / 4;  // at least four half blocks per workgroup
        if (nsplit < 1) nsplit = 1;
        a.per = (total + nsplit - 1) / nsplit;
        nsplit = (total + a.per - 1) / a.per;
        a.slab = base + slab0 * stride;
        a.slab_stride = stride;
        a.bias = j.dbias != nullptr;
        red.push_back(RedJob{a.slab, nsplit, stride, (int64_t)TMW * TNW, j.rows, j.cols, TNW, j.ldd, j.dst, j.dbias});
        slab0 += nsplit;
        nsplit_max = nsplit > nsplit_max ? nsplit : nsplit_max;
        double rows = 0;
        for (int i = 0; i < j.nseg; ++i) rows += 16.0 * (double)j.seg[i].nhalf;
        flops += 2.0 * rows * j.rows * j.cols;
    }
    if (used + slab0 * stride > work_floats) return PN_ERR_BAD_SHAPE;
    used += slab0 * stride;
    // (a job with fewer workgroups than grid.x: its surplus workgroups find h0 >= half_total and return before any store - they
    // have no slab; the reduction reads the job's own nsplit slabs)
    const dim3 grid((unsigned)nsplit_max, (unsigned)nj);
    const WgJob& j = j0;
    const WgMulti& a = m;
    {
    // (class per kernel instantiation: 6 + cfg; the Q24 forms of the 256 x 256 tile are 11 (Y in Q24) and 12 (X and Y in Q24))
    PnProfScope prof((j.cfg == 0 && j.fmt) ? (j.fmt == 3 ? 12 : 11) : 6 + j.cfg, flops, s);  // the GEMM kernel alone
    switch (j.cfg) {
        case 0:
            if constexpr (kQ24<NP>) {
                if (j.fmt == 3) { hipLaunchKernelGGL((k_chain_wgrad<NP, 2, 4, 4, 2, true, true>), grid, dim3(512), 0, s, a); break; }
                if (j.fmt == 1) { hipLaunchKernelGGL((k_chain_wgrad<NP, 2, 4, 4, 2, false, true>), grid, dim3(512), 0, s, a); break; }
            }
            if (j.fmt != 0) return PN_ERR_UNSUPPORTED;
            hipLaunchKernelGGL((k_chain_wgrad<NP, 2, 4, 4, 2>), grid, dim3(512), 0, s, a);
            break;
        case 1: hipLaunchKernelGGL((k_chain_wgrad<NP, 1, 3, 8, 1>), grid, dim3(512), 0, s, a); break;
        // (128 x 288 by twelve waves of 1 x 3 tiles: as four waves of 1 x 9 it held 392 registers per lane - one wave per
        // SIMD, two register sets in flight - and ran 3.8 TB/s)
        case 2: hipLaunchKernelGGL((k_chain_wgrad<NP, 1, 3, 4, 3>), grid, dim3(768), 0, s, a); break;
        case 3: hipLaunchKernelGGL((k_chain_wgrad<NP, 1, 2, 1, 4>), grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((k_chain_wgrad<NP, 1, 1, 1, 4>), grid, dim3(256), 0, s, a); break;
    }
    }
    PN_CHECK_LAUNCH();
    return run_reduce(red, 0, red.size(), s);
}
// the slab reductions of jobs [i0, i1) in one launch
static int run_reduce(const std::vector<RedJob>& red, size_t i0, size_t i1, hipStream_t s) {
    while (i0 < i1) {
        const size_t n = i1 - i0 < (size_t)RED_MAXJ ? i1 - i0 : (size_t)RED_MAXJ;
        RedMulti r{};
        int nmax = 0;
        for (size_t q = 0; q < n; ++q) {
            r.job[q] = red[i0 + q];
            const int e = r.job[q].rows * r.job[q].cols + (r.job[q].dbias ? r.job[q].rows : 0);
            nmax = e > nmax ? e : nmax;
        }
        hipLaunchKernelGGL(k_reduce_job, dim3((unsigned)((nmax + 63) / 64), (unsigned)n), dim3(256), 0, s, r);
        PN_CHECK_LAUNCH();
        i0 += n;
    }
    return PN_OK;
}

extern "C" {

int64_t pn_chain_wgrad_work_floats(void) {
    // the partial sums of one launch (a group of jobs of one tile configuration): (workgroups) x (tile + row sums) floats, the
    // largest being one 256 x 256 slab per CU; sized for up to 320 CUs
    const int64_t stride = 256 * 288 + 256;
    return (256 + 64) * stride + 1024;
}

/* Weight and bias gradients of ONE training step from the T32 tensors the chain kernels left behind: one split-bf16
 * (or plain bf16) TN GEMM per layer over the sample blocks of all `n` evaluations (and, for an evaluation with
 * rs_t / tang_t, its second-order rows r_l^T hdot_{l-1}); accumulates (+=) into the flat gradient block. */
int pn_chain_wgrad(int n, const PnChainEval* ev, int nc, int planes, float* grads, float* work, int64_t work_floats,
                   int which, int t_format, int max_wgs, void* stream) {
    if (n < 1 || n > 3 || which < 1 || which > 3 || max_wgs < 0) return PN_ERR_BAD_SHAPE;
    if (!tfmt_ok(planes, t_format)) return PN_ERR_UNSUPPORTED;
    const bool first = which & 1, second = which & 2;
    if (nc != 1 && nc != 5) return PN_ERR_UNSUPPORTED;
    if (planes != 1 && planes != 2 && planes != 3) return PN_ERR_UNSUPPORTED;
    if (!ev || !grads || !work) return PN_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    const PnLayout L = pn_layout(nc);
    int n2 = 0;
    for (int e = 0; e < n; ++e) {
        if (ev[e].M <= 0 || !ev[e].enc_t || !ev[e].acts_t) return PN_ERR_NULL;
        if (first && (!ev[e].drgb_t || !ev[e].dhv_t || !ev[e].d8_t || !ev[e].delta_t)) return PN_ERR_NULL;  // (written by the backward chain)
        if (ev[e].rs_t) {
            if (!ev[e].edot_t || !ev[e].tang_t || (first && !ev[e].coef_t)) return PN_ERR_NULL;
            if (second) ++n2;
        }
        if (planes == 2 && !ev[e].amax) return PN_ERR_NULL;
    }
    if ((first ? n : 0) + n2 > 4) return PN_ERR_UNSUPPORTED;
    if (!first && !n2) return PN_OK;  // second-order rows only, and no evaluation has any
    // planes = 2: a weight gradient sums over ALL samples, so each operand tensor gets ONE power of two, from the maxima
    // the chain kernels left in the evaluation's table
    // the step's jobs are collected first and launched in groups of the same tile configuration and operand format (see WgMulti);
    // `after`: a job that adds into the destination of an earlier one (the softplus' row of the density head) goes in a later launch
    std::vector<WgJob> jobs;
    std::vector<int> after;
    auto run = [&](const WgJob& j, int later = 0) {
        if (j.nseg) {
            jobs.push_back(j);
            after.push_back(later);
        }
        return (int)PN_OK;
    };
    auto am = [&](int e, int slot) -> const uint32_t* { return ev[e].amax ? ev[e].amax + slot : nullptr; };
    auto mp = [&](int e) { return pn_pad(ev[e].M); };
    // the T tensors hold 2-byte elements with planes = 1 (see TEl): offsets are in ELEMENTS of the mode's type
    const int64_t esz = planes == 1 ? 2 : 4;
    auto at = [&](const float* p, int64_t elems) { return reinterpret_cast<const float*>(reinterpret_cast<const char*>(p) + elems * esz); };
    auto act = [&](int e, int slot) { return at(ev[e].acts_t, act_off(slot, mp(e))); };
    int rc;
    // trunk layers (layer 5: hidden columns here, skip columns below)
    for (int l = 0; l < 8; ++l) {
        WgJob j{};
        for (int e = 0; e < n; ++e) {
            const int64_t Mp = mp(e);
            if (first)
                j.seg[j.nseg++] = WSeg{at(ev[e].delta_t, (int64_t)l * Mp * 256), l == 0 ? ev[e].enc_t : act(e, l - 1), Mp / 16, 256,
                                       l == 0 ? 96 : 256, 1, am(e, AM_DELTA0 + l), am(e, l == 0 ? AM_ENC : AM_ACT0 + l - 1)};
            if (second && ev[e].rs_t)
                j.seg[j.nseg++] = WSeg{at(ev[e].rs_t, (int64_t)l * Mp * 256),
                                       l == 0 ? ev[e].edot_t : at(ev[e].tang_t, (int64_t)(l - 1) * Mp * 256), Mp / 16, 256,
                                       l == 0 ? 96 : 256, 0, am(e, AM_RS0 + l), am(e, l == 0 ? AM_EDOT : AM_TANG0 + l - 1)};
        }
        j.cfg = l == 0 ? 1 : 0;
        // fp16 pairs: delta_l / r_l (l = 1-4, 6, 7) and h_{l-1} / hdot_{l-1} (l >= 1) come in Q24
        j.fmt = (t_format == 1 && l >= 1) ? (q24_delta(l) ? 3 : 1) : 0;
        j.rows = 256;
        j.cols = l == 0 ? 96 : 256;
        j.dst = grads + L.w[l];
        j.ldd = l == 0 ? 96 : (l == 5 ? 352 : 256);
        j.dbias = first ? grads + L.b[l] : nullptr;
        if ((rc = run(j)) != PN_OK) return rc;
        if (l == 5) {
            WgJob k{};
            for (int e = 0; e < n; ++e) {
                const int64_t Mp = mp(e);
                if (first)
                    k.seg[k.nseg++] = WSeg{at(ev[e].delta_t, (int64_t)5 * Mp * 256), ev[e].enc_t, Mp / 16, 256, 96, 0,
                                           am(e, AM_DELTA0 + 5), am(e, AM_ENC)};
                if (second && ev[e].rs_t)
                    k.seg[k.nseg++] = WSeg{at(ev[e].rs_t, (int64_t)5 * Mp * 256), ev[e].edot_t, Mp / 16, 256, 96, 0,
                                           am(e, AM_RS0 + 5), am(e, AM_EDOT)};
            }
            k.cfg = 1; k.rows = 256; k.cols = 96;
            k.dst = grads + L.w[5] + 256; k.ldd = 352; k.dbias = nullptr;
            if ((rc = run(k)) != PN_OK) return rc;
        }
    }
    if (first) {  // extra layer: d bottleneck^T h7
        WgJob j{};
        for (int e = 0; e < n; ++e) j.seg[j.nseg++] = WSeg{ev[e].d8_t, act(e, 7), mp(e) / 16, 288, 256, 1, am(e, AM_D8B), am(e, AM_ACT0 + 7)};
        j.cfg = 0; j.rows = 256; j.cols = 256; j.dst = grads + L.we; j.ldd = 256; j.dbias = grads + L.be;
        if ((rc = run(j)) != PN_OK) return rc;
    }
    {  // density head: d raw_density^T h7 (+ softplus' rows against hdot_7 into row 0)
        WgJob j{};
        if (first)
            for (int e = 0; e < n; ++e) j.seg[j.nseg++] = WSeg{at(ev[e].d8_t, 256 * TILE), act(e, 7), mp(e) / 16, 288, 256, 1, am(e, AM_D8D), am(e, AM_ACT0 + 7)};
        j.cfg = 3; j.rows = nc; j.cols = 256; j.dst = grads + L.wd; j.ldd = 256; j.dbias = grads + L.bd;
        if ((rc = run(j)) != PN_OK) return rc;
        WgJob k{};  // (with the first-order products: coef_t is written by the evaluation's backward chain)
        for (int e = 0; e < n; ++e)
            if (first && ev[e].rs_t)
                k.seg[k.nseg++] = WSeg{ev[e].coef_t, at(ev[e].tang_t, (int64_t)7 * mp(e) * 256), mp(e) / 16, 32, 256, 0,
                                       am(e, AM_COEF), am(e, AM_TANG0 + 7)};
        if (k.nseg) {
            k.cfg = 3; k.rows = 1; k.cols = 256; k.dst = grads + L.wd; k.ldd = 256; k.dbias = nullptr;
            if ((rc = run(k, 1)) != PN_OK) return rc;
        }
    }
    if (first) {  // view layer: d hv^T [bottleneck | view encoding]
        WgJob j{};
        for (int e = 0; e < n; ++e) j.seg[j.nseg++] = WSeg{ev[e].dhv_t, act(e, 8), mp(e) / 16, 128, 288, 1, am(e, AM_DHV), am(e, AM_ACT0 + 8)};
        j.cfg = 2; j.rows = 128; j.cols = PN_WIDTH + PN_VIEW_DIM; j.dst = grads + L.wv; j.ldd = PN_WIDTH + PN_VIEW_DIM;
        j.dbias = grads + L.bv;
        if ((rc = run(j)) != PN_OK) return rc;
    }
    if (first) {  // colour head: d rgb^T hv
        WgJob j{};
        for (int e = 0; e < n; ++e) j.seg[j.nseg++] = WSeg{ev[e].drgb_t, act(e, 9), mp(e) / 16, 32, 128, 1, am(e, AM_DRGB), am(e, AM_ACT0 + 9)};
        j.cfg = 4; j.rows = 3; j.cols = 128; j.dst = grads + L.wc; j.ldd = 128; j.dbias = grads + L.bc;
        if ((rc = run(j)) != PN_OK) return rc;
    }
    // Jobs share a launch only as far as a workgroup's range stays within WG_RANGE half blocks (8192 samples: what one job alone
    // gives a workgroup at the 4096-ray batch).  Sharing pays where the jobs are short - the 512-ray share of an 8-GPU run: 3.36 ->
    // 3.22 - 3.27 ms per step, nothing at 4096 rays (profiles/r04_multijob_ab.txt) - and a range n times as long is an n times
    // longer fp32 accumulation chain per accumulator: on the cancelling-sum stress test (1.97 M rows, fp32 tensors, seven jobs in
    // one launch) the error grew from 1.9e-6 to 7.4e-6 of the tensor's largest element (an fp32 GEMM: 1.5e-5).
    constexpr int64_t WG_RANGE = 512;
    std::vector<char> done(jobs.size(), 0);
    for (int pass = 0; pass < 2; ++pass)
    for (size_t i = 0; i < jobs.size(); ++i) {
        if (done[i] || after[i] != pass) continue;
        WgJob grp[WG_MAXJ];
        int ng = 0;
        int64_t total_i = 0;
        for (int q = 0; q < jobs[i].nseg; ++q) total_i += jobs[i].seg[q].nhalf;
        int cus_i = chain_cus();
        if (max_wgs > 0 && max_wgs < cus_i) cus_i = max_wgs;
        int64_t gmax = WG_RANGE * cus_i / (total_i > 0 ? total_i : 1);
        gmax = gmax < 1 ? 1 : (gmax > WG_MAXJ ? WG_MAXJ : gmax);
        for (size_t k = i; k < jobs.size() && ng < gmax; ++k)
            if (!done[k] && jobs[k].cfg == jobs[i].cfg && jobs[k].fmt == jobs[i].fmt && after[k] == after[i]) {
                grp[ng++] = jobs[k];
                done[k] = 1;
            }
        rc = planes == 3 ? run_wgrad_group<3>(grp, ng, work, work_floats, max_wgs, s)
                         : (planes == 2 ? run_wgrad_group<2>(grp, ng, work, work_floats, max_wgs, s)
                                        : run_wgrad_group<1>(grp, ng, work, work_floats, max_wgs, s));
        if (rc != PN_OK) return rc;
    }
    return PN_OK;
}

}  // extern "C"
