// pn_chain.h - what the two kernel families of the fused MLP share: the chain kernels (pn_chain.hip: forward, reverse sweep,
// tangent sweep, backward) write the T tensors and their maxima, the weight-gradient GEMMs (pn_wgrad.hip) read them back.
//
// Instruments (compile-time, never in the shipped build; tools/build_variant.sh builds both files with the same defines):
//   -DPN_ABL_CHAIN=<bits>   timing ablations of the chain GEMM step (WRONG results): bit 0 no refill DMA, bit 1 no fragment reads,
//                           bit 2 no MFMAs, bit 3 no ring barrier, bit 4 no T-layout stores
//   -DPN_ABL_WG=<bits>      timing ablations of the weight-gradient tile (WRONG results): bit 0 no matrix products, bit 1 no
//                           staging (the loaded registers are only consumed), bit 2 no barriers
//   -DPN_TRACE_CHAIN        shader-clock stamps of workgroup 0 of the chain kernels, read back with pn_chain_trace_read
//                           (tools/experiments/trace_chain.py); with it the environment variable PN_TRACE_ONE_WG=1 is honoured
//   -DPN_TRACE_WG           phase times of workgroup 0 of the 256 x 256 weight-gradient tile on Q24 operands, same reader
//                           (tools/experiments/trace_wgrad.py)
// The two traces share the reader's name: one of them per build.
#pragma once
#include "pn_common.h"
#include <math.h>
#include <string.h>
#include <stdlib.h>
#include <type_traits>
#include <utility>
#include <vector>

#if defined(PN_TRACE_CHAIN) && defined(PN_TRACE_WG)
#error "PN_TRACE_CHAIN and PN_TRACE_WG both define pn_chain_trace_read: one trace per build"
#endif
#ifndef PN_ABL_CHAIN
#define PN_ABL_CHAIN 0
#endif
#ifndef PN_ABL_WG
#define PN_ABL_WG 0
#endif

// f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N - 1>{}): a loop whose index is a constant expression
// in the body (immediate operands of inline asm)
template <typename F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int TILE = 16;  // samples per wave = features per accumulator tile = samples per T-layout block

// Element type of the T tensors: fp32, except with plain bf16 operands (NP = 1), where the value that is stored is the
// very bf16 the next GEMM and the weight-gradient GEMM consume - storing it in 2 bytes loses nothing and halves the HBM
// traffic of a mode that is HBM-bound.
template <int NP>
struct TEl {
    typedef float type;
};
template <>
struct TEl<1> {
    typedef __bf16 type;
};
template <int NP>
struct PlaneOf {
    typedef bf16x8 type;
};
template <>
struct PlaneOf<2> {
    typedef f16x8 type;
};
template <int NP>
struct BFrag {
    typename PlaneOf<NP>::type p[NP];
};

// NP = 2 only: one power-of-two scale per packed GEMM, 2^wexp, that takes the largest |weight| of its segments into
// [2^14, 2^15) (fp16 holds 65504).  Exponents are capped from above only - +30 for a weight matrix, +80 for a sample's
// vector or a tensor (zeros, or magnitudes below 2^-66 = 1.4e-20, which then lose precision gradually): a bias enters a
// sum as bias * 2^(wexp + bex) and must stay inside fp32's range; large values are never capped, they scale down.
constexpr int EXP_TOP = 15;    // frexp exponent of the scaled maximum
constexpr int EXP_CAP = 80;    // samples / tensors of the forward chain (its sums start from a bias)
constexpr int EXP_CAP_W = 30;  // weight matrices
constexpr int EXP_CAP_Z = 120; // samples / tensors of the backward-direction chains and of the weight gradients: their sums
                               // start at zero, so only the operands' own range matters (deltas of 1e-30 keep full precision)
__device__ __forceinline__ int scale_exp(float amax, int cap = EXP_CAP) {
    const int e = EXP_TOP - __builtin_amdgcn_frexp_expf(amax);
    return e > cap ? cap : e;
}

// NP = 2: x * 2^ex = h + l in fp16 (11 + 11 significant bits and the sign of l: the error is below 2^-24 |x| while
// l stays normal, and below 2^-39 of the column's largest element otherwise); NP = 3: x = h + m + l in bf16, exactly.
// The fp16 pairs of two elements, packed: h = fl16(x s), l = fl16(x s - h) for a power of two s, by mixed-precision FMAs
// that round once into their half of the destination - two instructions per element where ldexp, convert, convert
// back, subtract, convert take 3.5 (bit-identical to that sequence up to the sign of a zero; the chain kernels and the
// weight-gradient GEMMs are bound by their vector + matrix instruction time, and the split is a third of the former).
// N pairs at once (pair q: h[q], l[q] <- x[2 q], x[2 q + 1]), one of the four steps for all pairs before the next: every instruction of a pair reads the register the
// previous one wrote (half-register writes), which costs a wait state (an s_nop 0, as expensive to issue as the FMA) when the
// two are adjacent - written pair by pair the split ran 3.5 issue slots per element instead of 2.
template <int N>
__device__ __forceinline__ void split2_pairs(const float (&x)[2 * N], float s, uint32_t (&h)[N], uint32_t (&l)[N]) {
#pragma unroll
    for (int q = 0; q < N; ++q) asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h[q]) : "v"(x[2 * q]), "v"(s));
#pragma unroll
    for (int q = 0; q < N; ++q) asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h[q]) : "v"(x[2 * q + 1]), "v"(s));
#pragma unroll
    for (int q = 0; q < N; ++q)
        asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(l[q]) : "v"(x[2 * q]), "v"(s), "v"(h[q]));
#pragma unroll
    for (int q = 0; q < N; ++q)
        asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l[q]) : "v"(x[2 * q + 1]), "v"(s), "v"(h[q]));
}
__device__ __forceinline__ float pow2f(int e) { return __int_as_float((127 + e) << 23); }  // -126 <= e <= 127

// slots of an evaluation's table of maxima (uint32 float bits, AM_COUNT per evaluation)
enum {
    AM_ENC = 0, AM_ACT0 = 1 /* h0..h7, [bottleneck | view encoding], view hidden */, AM_DELTA0 = 11 /* delta_0..7 */,
    AM_D8B = 19, AM_D8D = 20, AM_DHV = 21, AM_DRGB = 22, AM_RS0 = 23 /* r_0..7 */, AM_TANG0 = 31 /* hdot_0..7 */,
    AM_EDOT = 39, AM_COEF = 40, AM_COUNT = 64
};

// ---- Q24: a T tensor in THREE bytes per element (round 3) --------------------------------------------------------------
// The tensors that only the weight-gradient GEMMs read back - h0..h6, hdot_0..6, delta_l and r_l for l = 1-4, 6, 7: 26 of the
// 32 KB a second-order evaluation writes per sample in its 256-wide vectors - are stored as fp32 ROUNDED TO 16 SIGNIFICANT BITS,
// the four features of a quad block of a sample in 12 bytes: [block][F / 4][16 samples][12 B].  A quad block of a lane is ONE
// 12-byte store (768 contiguous bytes per wave instruction) where four dword stores stood, and a quarter of the bytes of the
// step's HBM traffic in these tensors is gone on both sides - the chains' exposed store time and the weight-gradient GEMMs' read
// time follow the BYTES (profiles/r03_experiments.txt sections 9, 11, 13).  A 2^-17 rounding error per operand leaves a sum
// over samples ~1e-6 of its tensor's largest element off, the level of an fp32 GEMM's own summation noise (3e-6 on the same
// data: tests/test_gpu_chain.py::test_large_weight_gradient_sums_against_fp64_and_an_fp32_gemm); what the chains re-read
// themselves (encodings, r_5, delta_5) and the narrow tensors stay fp32.  fp16 pairs only; t_format = 0 of the entry points
// (mlp_mode "fused_f16x2_t32") keeps every T tensor fp32 for A/B measurements.
template <int NP>
constexpr bool kQ24 = NP == 2;
__host__ __device__ constexpr bool q24_act(int slot) { return slot <= 6; }                  // h_l / hdot_l
__host__ __device__ constexpr bool q24_delta(int slot) { return slot != 0 && slot != 5; }   // delta_l / r_l
// acts_t of an evaluation: h0..h7 [256] x 8, then [bottleneck | view encoding] [288], then the view hidden vector [128]
__host__ __device__ constexpr int64_t act_off(int slot, int64_t Mp) {  // float offset of activation slot in acts_t
    return slot <= 8 ? (int64_t)slot * Mp * 256 : 8 * Mp * 256 + Mp * 288;
}

// ---- host side: per-device launch state (a process may drive several devices, one host thread per device) ---------------------
constexpr int PN_MAX_DEVICES = 64;
inline int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= PN_MAX_DEVICES) dev = 0;
    return dev;
}
// CU count of every device, asked once per process (inline: ONE table, whichever translation unit asks first)
inline int g_chain_cus[PN_MAX_DEVICES] = {};
inline int chain_cus() {
    const int dev = current_device();
    if (!g_chain_cus[dev]) {
        hipDeviceProp_t pr;
        g_chain_cus[dev] = hipGetDeviceProperties(&pr, dev) == hipSuccess ? pr.multiProcessorCount : 256;
    }
    return g_chain_cus[dev];
}
// T-tensor format of a call: 0 = every tensor fp32 (bf16 with planes = 1), 1 = Q24 where pn_chain_q24_slots says so (fp16 pairs only)
inline bool tfmt_ok(int planes, int t_format) { return t_format == 0 || (t_format == 1 && planes == 2); }
