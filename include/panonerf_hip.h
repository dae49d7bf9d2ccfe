/*
 * panonerf_hip.h — C ABI of libpanonerf_hip.so (gfx950 / MI355X).
 *
 * The reference (Lu-Zhan/Pano-NeRF) has no FFI: its hot path is ATen op chains
 * inside Python functions.  Each entry point below replaces one such chain; the
 * reference file:line it stands in for is cited per function.  The Python module
 * pano_nerf_amd binds these through ctypes (see INTEGRATION.md for the stub a
 * maintainer of the reference would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32, row-major, contiguous, unless the
 *     parameter name ends in _host; the caller owns all device memory and the library
 *     allocates none;
 *   - process model: one host thread per device (how the reference runs under DDP).  No entry
 *     point keeps results or configuration between calls: every operand, workspace and packed
 *     weight block is passed in.  The only process-wide host state is bookkeeping that never
 *     reaches a result: the pool of hipEvent_t used to fork / join the optional side stream and
 *     by the opt-in launch timing (pn_prof_*), the cached CU count of the device, and one flag
 *     per kernel recording that its dynamic-LDS attribute has been set;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and the
 *     call returns without synchronising (graph-capturable);
 *   - return value: 0 on success, negative PN_ERR_* otherwise (the Python shim
 *     raises RuntimeError(pn_strerror(code)));
 *   - B rays, N samples per ray, S = N + 1 fence posts, M = B*N sample rows.
 *     Sample-row buffers written by the GEMM kernels must be allocated with
 *     pn_pad_rows(M) rows.
 */
#ifndef PANONERF_HIP_H
#define PANONERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PN_OK 0
#define PN_ERR_BAD_SHAPE (-1)   /* a size is <= 0 or violates a documented bound   */
#define PN_ERR_UNSUPPORTED (-2) /* e.g. N > PN_MAX_SAMPLES, density channels not 1/5 */
#define PN_ERR_NULL (-3)        /* a required pointer is null                       */
#define PN_ERR_HIP (-4)         /* a HIP launch failed (hipGetLastError != success) */

#define PN_MAX_SAMPLES 512 /* fence posts per ray handled by one wave: S <= 513 */
#define PN_ENC_DIM 96      /* 2 * 3 * (max_deg_point - min_deg_point), degrees 0..15 */
#define PN_VIEW_DIM 27     /* 3 + 2 * 3 * deg_view, deg_view = 4 */
#define PN_WIDTH 256
#define PN_WIDTH_COND 128
#define PN_ROW_PAD 128

const char* pn_strerror(int code);
int pn_abi_version(void);
/* rows a [M, *] sample buffer must be allocated with (M rounded up to PN_ROW_PAD) */
int64_t pn_pad_rows(int64_t m);

/* ---- flat parameter block --------------------------------------------------------
 * The 24 tensors of MLP / PureMLP (models/pano_mip_nerf.py:35-76, models/mip_nerf.py:19-60)
 * live in ONE fp32 block so that gradient all-reduce and Adam are one pass each.
 * Order: layers.0..7 {weight,bias}, extra_layer {w,b}, view_layers.0.0 {w,b},
 * density_layer.weight, color_layer.weight, density_layer.bias, color_layer.bias.
 * pn_param_layout fills offsets[24] (in floats, same order as above) and returns the
 * total float count (613768 for nc = 5, 612740 for nc = 1), or a negative error. */
int64_t pn_param_layout(int num_density_channels, int64_t* offsets_host);

/* workspace (floats) pn_pack_weights needs: transposed / split copies of the weights */
int64_t pn_wpack_floats(int num_density_channels);
/* (re)build the packed weights from the flat parameter block; call after every
 * optimizer step.  Replaces nothing upstream (ATen reads nn.Linear.weight directly). */
int pn_pack_weights(const float* params, int num_density_channels, float* wpack, void* stream);

/* ---- ray generation ----------------------------------------------------------------
 * PanoDataset._generate_rays, datasets/pano_datasets.py:152-216 (== sample_dir_by_pano,
 * utils/sampling.py:5-20).  One camera; outputs are [H*W, C] with C = 3,3,3,1,1,1,1,1. */
int pn_raygen_pano(int H, int W, const float* c2w_host /*[16] row-major 4x4*/, float near_, float far_,
                   float* origins, float* directions, float* viewdirs, float* radii, float* lossmult,
                   float* near_out, float* far_out, float* noise_var, void* stream);
/* PanoDataset.generate_lit_rays, datasets/pano_datasets.py:218-263 (== sample_dir_by_unifrom,
 * utils/sampling.py:23-38): fp64 math, stored as IEEE half.  out_half: 14*D uint16 laid out as
 * origins[D,3] directions[D,3] viewdirs[D,3] radii[D] lossmult[D] near[D] far[D] noise_var[D]. */
int pn_lit_rays(int D, double radius, double near_, double far_, uint16_t* out_half, void* stream);

/* Training-batch gather out of a device-resident ray pool — the host-side __getitem__ gather of
 * datasets/pano_datasets.py:271-275 (one DataLoader worker per 56-byte ray upstream).
 *   idx [B] int64 (device): pool row of every batch ray (out-of-range rows read row 0);
 *   pool_host / out_host: HOST arrays of 9 device pointers in the order origins, directions, viewdirs [.,3],
 *   radii, lossmult, near, far, noise_var [.,1], rgb [.,3]; entry 8 (rgb) may be null in both. */
int pn_gather_rays(int64_t B, int64_t pool_rays, const int64_t* idx, const float* const* pool_host,
                   float* const* out_host, void* stream);

/* Training-batch sampler that REGENERATES the rays instead of reading a stored pool (replaces
 * PanoDataset.__getitem__, datasets/pano_datasets.py:271-275, over the pool of _generate_rays, :152-216): batch ray b is
 * pixel idx[b] % (H W) of camera idx[b] / (H W), computed with the arithmetic of pn_raygen_pano (bit-identical to a
 * gather out of its output).  c2ws: DEVICE [n_cam,16] row-major 4x4; rgb_pool [n_cam H W,3] / rgb_out [B,3]: target
 * colours, both or neither; out-of-range idx reads ray 0. */
int pn_sample_pano_rays(int64_t B, int n_cam, int H, int W, const int64_t* idx, const float* c2ws, float near_, float far_,
                        const float* rgb_pool, float* origins, float* directions, float* viewdirs, float* radii,
                        float* lossmult, float* near_out, float* far_out, float* noise_var, float* rgb_out, void* stream);

/* ---- sampling ----------------------------------------------------------------------
 * sample_along_rays (models/mip.py:113-151; disparity != 0: positions linear in inverse depth, :134-136) + cast_rays (67-89) +
 * conical_frustum_to_gaussian (36-64, stable) + lift_gaussian (8-22, diagonal).
 * t_rand: [B,S] uniforms or null (deterministic). */
int pn_sample_coarse(int64_t B, int N, int disparity, const float* origins, const float* directions, const float* radii,
                     const float* near_, const float* far_, const float* t_rand, float* t_out, float* mean,
                     float* cov, void* stream);
/* resample_along_rays (models/mip.py:304-352, stop_grad branch) + sorted_piecewise_constant_pdf
 * (240-301) + cast_rays.  u_rand: [B,S] uniforms in [0, 1/S - eps) or null. */
int pn_resample(int64_t B, int N, const float* t_in, const float* weights, float padding, const float* u_rand,
                const float* origins, const float* directions, const float* radii, float* t_out, float* mean,
                float* cov, void* stream);
/* sample_each_points (models/mip.py:154-194) for x_surf = origins + directions * distance
 * (models/pano_mip_nerf.py:324-334).  Light ray r = b*D + j.  env_rand: [Ne+1] uniforms or null.
 * env_dirs/env_radii/env_near/env_far: [D,*] fp32 (fp16-rounded values up-cast by the caller). */
int pn_sample_env(int64_t B, int D, int Ne, const float* origins, const float* directions, const float* distance,
                  const float* env_dirs, const float* env_radii, const float* env_near, const float* env_far,
                  const float* env_rand, float* t_out /*[B*D,Ne+1]*/, float* mean /*[B*D*Ne,3]*/,
                  float* cov /*[B*D*Ne,3]*/, void* stream);

/* ---- encodings ---------------------------------------------------------------------
 * integrated_pos_enc (models/mip.py:394-428, diagonal) -> enc [Mpad,96] */
int pn_ipe_encode(int64_t M, const float* mean, const float* cov, float* enc, void* stream);
/* pos_enc (models/mip.py:431-441, min_deg 0, max_deg 4, identity prepended) -> [R,27] */
int pn_pos_enc_view(int64_t R, const float* viewdirs, float* viewenc, void* stream);

/* ---- MLP ---------------------------------------------------------------------------
 * MLP.forward / PureMLP.forward (models/pano_mip_nerf.py:95-114, models/mip_nerf.py:81-102).
 * Rows are samples; sample row i belongs to view row (i / rows_per_ray) % view_mod
 * (view_mod = number of rows of viewdirs).  acts: [PN_ACT_SLOTS][Mpad,256] saved activations
 * (h0..h7, bottleneck, view hidden [.,128 used]) — required (backward and the density
 * gradient re-read them).  enc: [Mpad,96] (written).  viewenc: [view_rows,27] (written),
 * viewbias: [view_rows,128] scratch. */
#define PN_ACT_SLOTS 10
/* masks: [PN_MASK_SLOTS][Mpad][PN_MASK_WORDS] u32 — ReLU gates of h0..h7 and the view hidden as bit masks
 * (written here, read by pn_density_grad / pn_mlp_backward: 32 B/row instead of re-reading 1 KB/row). */
#define PN_MASK_SLOTS 9
#define PN_MASK_WORDS 8
int pn_mlp_forward(int64_t M, int rows_per_ray, int64_t view_rows, int num_density_channels, const float* params,
                   const float* wpack, const float* mean, const float* cov, const float* viewdirs, float* enc,
                   float* viewenc, float* viewbias, float* acts, uint32_t* masks, float* raw_rgb /*[M,3]*/,
                   float* raw_density /*[M,nc]*/, void* stream);

/* d sigma / d mean per sample: what vmap(jacrev(compute_graph))[1] keeps
 * (models/pano_mip_nerf.py:299-303, models/mip_nerf.py:261-265), computed as ONE reverse
 * sweep seeded with softplus'(raw_density0 + bias) * density_layer.weight[0].
 * rsweep: [8][Mpad,256] saved sweep vectors (needed by pn_mlp_backward's second-order term);
 * scratch: [Mpad,96].  Output grad_mean [M,3] = + d sigma / d mean (caller negates). */
int pn_density_grad(int64_t M, int num_density_channels, float density_bias, const float* params,
                    const float* wpack, const float* mean, const float* cov, const float* acts,
                    const uint32_t* masks, const float* raw_density, float* rsweep, float* scratch,
                    float* grad_mean, void* stream);

/* Backward of pn_mlp_forward (+ optionally of pn_density_grad).  Accumulates (+=) into
 * `grads` (flat block, layout of pn_param_layout).
 *   d_raw_rgb [M,3], d_raw_density [M,nc]: upstream gradients;
 *   v_gradmean [M,3] or null: upstream gradient w.r.t. pn_density_grad's output (second-order
 *     path: needs rsweep from pn_density_grad; d_raw_density[:,0] receives the
 *     softplus'' term internally);
 *   d_mean [M,3] or null: if non-null receives d loss / d mean (first-order, env-light path).
 * M is a whole number of rays (M % rows_per_ray == 0) and the rays cycle through the view rows
 * ((M / rows_per_ray) % view_rows == 0): ray r uses viewenc[r % view_rows], as in pn_mlp_forward.
 * work: scratch of pn_mlp_backward_work_floats(M, rows_per_ray, view_rows, M_batched) floats.
 * Batching the weight gradients of one training step: the evaluations of a step (env light, level 1, level 0) share
 * the weights, so their trunk / extra-layer weight gradients are ONE TN GEMM per layer over all their rows.  Calls with
 * defer_wgrad = 1 skip those GEMMs and leave their operands in `work` (keep it alive); the last call passes
 * n_deferred (<= 2) and, per deferred evaluation, its M, enc, acts, rsweep (or null), work and whether it ran the
 * tangent sweep (host arrays), and reduces everything.  M_batched = total rows of those GEMMs (own + deferred, tangent
 * rows counted) sizes the slab part of `work` (0 = stand-alone).
 * The kept head of `work`, which a later call reads through dwork_host and which holds these results after every call
 * (Mp = pn_pad_rows(M), rows >= M are not written), in this order from its first float:
 *   delta [9][Mp][256]  d loss / d pre-activation of h0..h7; slot 8: the density-head addend d_raw_density * Wd
 *   tang  [8][Mp][256]  the tangent sweep hdot_0..hdot_7 (written only with v_gradmean)
 *   d_bott   [Mp][256]  d loss / d bottleneck
 *   edot     [Mp][96]   the tangent of the encoding along v_gradmean (written only with v_gradmean)
 * Everything behind it is scratch whose layout is private to the call.
 * side_stream (nullable): a second hipStream_t; when given, the weight-gradient GEMMs / reductions run there,
 * forked from and joined back to `stream` with events inside the call, so they overlap the data-gradient chain. */
int64_t pn_mlp_backward_work_floats(int64_t M, int rows_per_ray, int64_t view_rows, int64_t M_batched);
int pn_mlp_backward(int64_t M, int rows_per_ray, int64_t view_rows, int num_density_channels, float density_bias,
                    const float* params, const float* wpack, const float* mean, const float* cov,
                    const float* enc, const float* viewenc, const float* acts, const uint32_t* masks,
                    const float* raw_density, const float* d_raw_rgb, const float* d_raw_density,
                    const float* rsweep, const float* v_gradmean, float* d_mean, float* grads, float* work,
                    int64_t M_batched, int defer_wgrad, int n_deferred, const int64_t* dM_host,
                    const float* const* denc_host, const float* const* dacts_host,
                    const float* const* drsweep_host, float* const* dwork_host, const int* dtangent_host,
                    void* stream, void* side_stream);


/* ---- fused on-chip MLP chains (pn_chain.hip; weight gradients: pn_wgrad.hip) ----------------------------------------
 * The same MLP (models/pano_mip_nerf.py:95-114, models/mip_nerf.py:81-102), encodings (models/mip.py:394-441) and
 * their reverse / forward-mode passes as ONE kernel per pass: every layer is computed transposed on
 * v_mfma_f32_16x16x32_bf16 / _f16, a wave carries the activations of its 16 samples from layer to layer in registers, the
 * weights stream through an LDS ring by LDS-DMA.  planes = 3: exact 3-term bf16 split, six partial products (fp32
 * accuracy); planes = 2: fp16 pairs (x 2^e = h + l, |error| < 2^-24 |x|), three partial products, one power-of-two scale
 * per weight matrix and per sample (chains) or per tensor (weight gradients), fp32 accumulate; planes = 1: plain bf16
 * operands, fp32 accumulate.  Sample-row tensors these kernels exchange are in the "T layout":
 * elem[Mp/tile][F][tile] (sample-minor, tile = pn_chain_tile(), Mp = pn_pad_rows(M)), elem = float for planes 3 and 2,
 * bf16 for planes = 1 (the stored value is the bf16 the next GEMM consumes: the float* parameters below then point at
 * 2-byte elements, and a buffer sized in floats is twice as large as needed); gate words are uint32 [9][Mp][8]
 * (per row: lane-group order, see pn_chain.hip; producers and consumers are all in this library). */
/* samples per block of the sample-minor tensors (= samples per wave of the chain kernels): 16 (v_mfma_f32_16x16x32, two
 * waves per SIMD).  Callers ask instead of assuming it.  Below, "T layout" means elem[Mp / tile][F][tile]. */
int pn_chain_tile(void);
/* "Q24": with planes = 2, the 256-wide tensors that only pn_chain_wgrad reads back are stored in THREE bytes per
 * element - fp32 rounded to 16 significant bits (round to nearest on the dropped byte), the four features of a quad block of a
 * sample in 12 bytes: elem[Mp / 16][F / 4][16][12 B], byte b of a feature's three = bits 8 (b + 1) .. 8 (b + 1) + 7 of the rounded
 * fp32 - a quarter of the step's HBM traffic in these tensors; each keeps its slot's address (slot * Mp * 256 floats) and uses the
 * first three quarters of it.  Bit s of the result: slot s of the tensor is Q24; tensor 0: activations h_s (acts_t), 1: tangents
 * hdot_s (tang_t), 2: deltas (delta_t), 3: reverse-sweep vectors r_s (rs_t).  0 for every other mode: all fp32 (or bf16). */
int pn_chain_q24_slots(int planes, int t_format, int tensor);
/* Two arguments every chain entry point below takes (ABI 2):
 *   t_format  0: every T tensor fp32 (bf16 with planes = 1); 1: Q24 where pn_chain_q24_slots says so (planes = 2 only).  The calls of
 *             one evaluation - forward, sweeps, backward, weight gradients - must agree on it: it is the layout of what they exchange.
 *   max_wgs   0: the launch sizes its persistent grid to every CU of the device.  > 0: it occupies at most that many workgroups (a chain
 *             workgroup or a 256-wide weight-gradient workgroup fills a CU), so that a kernel of the OTHER family, launched on another
 *             stream with the complementary budget, finds the remaining CUs free: the chains are bound by matrix-instruction issue and
 *             their stores (2.7 TB/s of HBM traffic), the weight gradients by their operand reads - side by side on disjoint CUs each
 *             sees less HBM contention than alone on the whole chip.  Results do not depend on it for the
 *             chains; for pn_chain_wgrad it moves the split points of the sum over samples (deterministic for a given value). */
int64_t pn_chain_pack_bytes(int planes);
int pn_chain_pack(const float* params, int num_density_channels, int planes, void* pack, void* stream);
/* floats of acts_t: h0..h7 [256] x 8, bottleneck | view encoding [288], view hidden [128].  acts_t may be NULL in
 * pn_chain_forward (inference: nothing re-reads the activations; enc_t and the gate words are still written). */
int64_t pn_chain_acts_floats(int64_t M);
/* amax (planes = 2, training; NULL otherwise): ONE evaluation's table of pn_chain_amax_slots() uint32, the largest |x| of
 * every T tensor the weight gradients will read (float bits).  pn_chain_forward clears it, the four chain kernels of the
 * evaluation add their tensors' maxima, pn_chain_wgrad derives one power-of-two scale per tensor from it. */
int pn_chain_amax_slots(void);
/* view_tab: scratch of view_rows * 32 floats - the view encoding (pos_enc, models/mip.py:431-441) depends on the view row
 * only, so it is evaluated once per row (a small kernel in front of the chain) and read by the row's samples. */
int pn_chain_forward(int64_t M, int rows_per_ray, int64_t view_rows, int num_density_channels, int planes,
                     const void* pack, const float* mean, const float* cov, const float* viewdirs, float* view_tab,
                     float* enc_t, float* acts_t, uint32_t* masks, float* raw_rgb /*[M,3]*/, float* raw_density /*[M,nc]*/,
                     uint32_t* amax, int t_format, int max_wgs, void* stream);
/* vmap(jacrev(compute_graph))[1] (models/pano_mip_nerf.py:299-303) as one reverse sweep.  keep_all != 0: rs_t is
 * T [8][Mp*256] and receives r_0..r_7 (the second-order weight gradients need them); keep_all = 0 (inference): rs_t is ONE
 * slot T [Mp*256], used only for the kernel's own reload of r_5. */
int pn_chain_density_grad(int64_t M, int num_density_channels, int planes, float density_bias, const float* params,
                          const void* pack, const float* mean, const float* cov, const uint32_t* masks,
                          const float* raw_density, float* rs_t, int keep_all, float* grad_mean /*[M,3]*/,
                          uint32_t* amax, int t_format, int max_wgs, void* stream);
/* forward-mode tangent sweep along v_gradmean (the double backward of the normals block) */
int pn_chain_tangent(int64_t M, int num_density_channels, int planes, const float* params, const void* pack,
                     const float* mean, const float* cov, const uint32_t* masks, const float* v_gradmean,
                     float* edot_t /*T [Mp*96]*/, float* tang_t /*T [8][Mp*256]*/, float* sdot /*[M]*/, uint32_t* amax,
                     int t_format, int max_wgs, void* stream);
/* data-gradient chain.  drgb_t T [Mp*32], d8_t T [Mp*288], coef_t T [Mp*32]: with pn_chain_tile() = 32 the caller
 * zero-fills them once (the kernel writes 16 of their 32 padded features); with the default 16 the kernel writes them
 * whole.  sdot / coef_t: second-order path (both or neither); d_mean nullable. */
int pn_chain_backward(int64_t M, int num_density_channels, int planes, float density_bias, const void* pack,
                      const uint32_t* masks, const float* raw_density, const float* d_raw_rgb,
                      const float* d_raw_density, const float* sdot, const float* mean, const float* cov,
                      float* drgb_t, float* dhv_t /*T [Mp*128]*/, float* d8_t, float* delta_t /*T [8][Mp*256]*/,
                      float* coef_t, float* d_mean /*[M,3]*/, uint32_t* amax, int t_format, int max_wgs, void* stream);
/* one evaluation's tensors for the weight gradients (host struct of device pointers) */
typedef struct PnChainEval {
    int64_t M;
    const float* enc_t;
    const float* acts_t;
    const float* drgb_t;
    const float* dhv_t;
    const float* d8_t;
    const float* delta_t;
    const float* rs_t;   /* second-order rows: all four or none */
    const float* edot_t;
    const float* tang_t;
    const float* coef_t;
    const uint32_t* amax; /* planes = 2: the evaluation's table of maxima; NULL otherwise */
} PnChainEval;
int64_t pn_chain_wgrad_work_floats(void);
/* which: bit 1 = the second-order TRUNK rows (r_l^T hdot_{l-1}, r_0^T edot) of the evaluations that carry rs_t - their operands exist as
 * soon as the tangent sweep has run, before the evaluation's backward chain, so a caller can reduce them under that chain on another
 * stream; bit 0 = everything else (delta_l^T h_{l-1}, heads incl. the softplus' row against hdot_7, view / colour layer, bias gradients).
 * grads is accumulated into (+=) by the job reductions, in launch order: concurrent calls on the same `grads` must share a stream. */
int pn_chain_wgrad(int n_evals, const PnChainEval* evals_host, int num_density_channels, int planes, float* grads,
                   float* work, int64_t work_floats, int which, int t_format, int max_wgs, void* stream);

/* ---- volumetric rendering ---------------------------------------------------------
 * compute_graph activations (models/pano_mip_nerf.py:273-278) + volumetric_rendering
 * (models/mip.py:444-483).  R rays of N samples; dirs [R or dir_mod, 3] (ray r uses
 * dirs[r % dir_mod]).  Outputs comp_rgb [R,3], distance [R], acc [R], weights [R,N]. */
int pn_composite_forward(int64_t R, int N, int num_density_channels, float density_bias, float rgb_padding,
                         int white_bkgd, const float* raw_rgb, const float* raw_density, const float* t,
                         const float* dirs, int64_t dir_mod, float* comp_rgb, float* distance, float* acc,
                         float* weights, void* stream);
/* adjoint: d_comp_rgb [R,3], d_distance [R] (nullable), d_weights [R,N] (nullable) ->
 * d_raw_rgb [R*N,3] (=), d_raw_density [R*N,nc] channel 0 (=; other channels untouched). */
int pn_composite_backward(int64_t R, int N, int num_density_channels, float density_bias, float rgb_padding,
                          int white_bkgd, const float* raw_rgb, const float* raw_density, const float* t,
                          const float* dirs, int64_t dir_mod, const float* d_comp_rgb, const float* d_distance,
                          const float* d_weights, float* d_raw_rgb, float* d_raw_density, void* stream);

/* ---- normals / albedo gather (models/pano_mip_nerf.py:296-317, mip_nerf.py:258-275) --
 * grad_mean [B*N,3] = d sigma/d mean; weights [B,N]; raw_density [B*N,nc].
 * normals_s = normalize(-grad_mean); normal = normalize(sum w^ n_s); ort_ray[b] = sum w^ relu(n_s.d)^2
 * (caller takes the mean over B); albedo = sum w^ (sigmoid(raw[1:4])*0.77+0.03) (nc = 5 only). */
int pn_surf_gather_forward(int64_t B, int N, int num_density_channels, const float* grad_mean,
                           const float* weights, const float* raw_density, const float* directions,
                           float* normal /*[B,3]*/, float* ort_ray /*[B] or null*/, float* albedo /*[B,3] or null*/,
                           void* stream);
/* adjoint: d_normal [B,3], d_ort_ray [B] (nullable), d_albedo [B,3] (nullable) ->
 * d_weights [B,N] (=), v_gradmean [B*N,3] (=), d_raw_density channels 1..3 (=, nc = 5). */
int pn_surf_gather_backward(int64_t B, int N, int num_density_channels, const float* grad_mean,
                            const float* weights, const float* raw_density, const float* directions,
                            const float* d_normal, const float* d_ort_ray, const float* d_albedo,
                            float* d_weights, float* v_gradmean, float* d_raw_density, void* stream);

/* ---- Lambertian surface rendering (utils/surface_rendering.py:104-126, 129-165) -------
 * env_rgb [B,D,3], albedo/normal [B,3], env_dirs [D,3], solid_angle [D].
 * -> surface_rgb (= diffuse) [B,3], shading [B,3]. */
int pn_surface_forward(int64_t B, int D, const float* env_rgb, const float* albedo, const float* normal,
                       const float* env_dirs, const float* solid_angle, float* diffuse, float* shading,
                       void* stream);
int pn_surface_backward(int64_t B, int D, const float* env_rgb, const float* albedo, const float* normal,
                        const float* env_dirs, const float* solid_angle, const float* d_diffuse,
                        const float* d_shading, float* d_env_rgb, float* d_albedo, float* d_normal, void* stream);
/* d x_surf -> d distance: d_distance[b] (+=) sum_{rows of ray b} d_mean[row] . directions[b]
 * (models/pano_mip_nerf.py:324; rows_per_ray = D*Ne). */
int pn_env_origin_backward(int64_t B, int rows_per_ray, const float* d_mean, const float* directions,
                           float* d_distance, void* stream);

/* ---- tone-mapped loss (utils/surface_rendering.py:319-344, systems/panonerf_system.py:17,44-67,
 * systems/mipnerf_system.py:24,37-45).  Per-ray partials are reduced in-kernel; `loss_terms`
 * receives [mse_coarse, mse_fine, mse_surface, chrom, mask_sum, total]; d_* receive the gradients of
 *   total = cw*mse_coarse + mse_fine + sw*mse_surface + chw*chrom     (ort term added by caller).
 * rgb_surface / albedo may be null (terms skipped).  work: >= 8 + 8*ceil(B/256) floats. */
int pn_tonemap_loss(int64_t B, const float* rgb_gt_hdr, const float* lossmult, const float* rgb_coarse,
                    const float* rgb_fine, const float* rgb_surface, const float* albedo, float coarse_w,
                    float surface_w, float chrom_w, float* loss_terms /*[8]*/, float* d_coarse, float* d_fine,
                    float* d_surface, float* d_albedo, float* work, void* stream);

/* ---- optimizer: Adam over the flat block (torch.optim.Adam defaults,
 * systems/base_system.py:82) ; grads are scaled by grad_scale first (1/world_size after a
 * sum all-reduce). */
int pn_adam_step(int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float lr,
                 float beta1, float beta2, float eps, int step, float grad_scale, void* stream);

/* same update with the step counter (incremented first) and the learning rate read from device memory, so the
 * call can be captured once in a HIP graph and replayed every step */
int pn_adam_step_dev(int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                     const float* lr_dev, float beta1, float beta2, float eps, int* step_dev, float grad_scale,
                     void* stream);

/* ---- building blocks exposed for tests / profiling ------------------------------------
 * C[M,N] = epi(A[M,K] * Bt[N,K]^T) on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * flags: 1 = +bias[N], 2 = relu, 4 = gate by (gate[row,col] > 0). lda/ldb/ldc/ldg in floats. */
int pn_gemm_nt(int64_t M, int N, int K, const float* A, int lda, const float* Bt, int ldb, float* C, int ldc,
               const float* bias, const float* gate, int ldg, int flags, void* stream);
/* C[N1,N2] = X[M,N1]^T * Y[M,N2] (split over rows, deterministic two-pass reduction);
 * accumulate != 0 adds into C.  work: pn_gemm_tn_work_floats(M, N1, N2) floats. */
int64_t pn_gemm_tn_work_floats(int64_t M, int N1, int N2);
int pn_gemm_tn(int64_t M, int N1, int N2, const float* X, int ldx, const float* Y, int ldy, float* C, int ldc,
               int accumulate, float* work, void* stream);

/* ---- evaluation metrics of a rendered panorama (utils/metrics.py; pn_metrics.hip) ----------------------------
 * Reductions over [C, H, W] equirectangular images, C = 1 or 3.  Element (c, i, j) of an operand is read at
 * p[c * cs + (i * W + j) * ps] (cs: channel stride, ps: pixel stride, in floats), so the [1, C, H, W] permuted views
 * that render_image returns are read in place.  Pixel weights are the solid angles sin((i + 1/2) pi / H), normalised
 * to sum 1 over the H x W pixels (utils/surface_rendering.py:294-316).  Tone mapping per operand (`*_tone`): 0 none,
 * 1 hdr_to_ldr(x), 2 hdr_to_ldr(x, dtype='uint8') (utils/surface_rendering.py:319-341).  Results are fp64 SUMS
 * written to `out` (device); means are formed by the caller.  Partial sums go to `work` (device, at least
 * pn_metrics_work_doubles(C, H, W) doubles) and are summed in a fixed order: no atomics, bit-reproducible.
 * A non-finite input propagates to the sums, as in torch.  Errors: PN_ERR_BAD_SHAPE (H or W <= 0, C not 1 or 3,
 * n <= 0), PN_ERR_UNSUPPORTED (unknown tone mode, window != 11, y_normalize not 0..2). */
int64_t pn_metrics_work_doubles(int C, int H, int W);
/* d = tone(x) - tone(y): out[6] = [sum d^2, sum |d|, sum w d^2, sum w |d|, sum d, element count] */
int pn_metric_sums(int C, int H, int W, const float* x, int64_t x_cs, int64_t x_ps, int x_tone, const float* y,
                   int64_t y_cs, int64_t y_ps, int y_tone, double* out, double* work, void* stream);
/* SSIM of tone(x) and tone(y) per channel (utils/metrics.py:44-200: 11 x 11 Gaussian window of sigma 1.5, zero
 * padding, C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2): out[3] = [sum s, sum w s (over channels), count];
 * taps: the window's 1-D factor, `window` (= 11) device doubles (the reference builds it as fp32
 * exp(-(k - 5)^2 / 4.5) over its fp32 sum; passing it in keeps every caller on the same bits);
 * map (nullable): the SSIM map, [C, H, W] contiguous fp32. */
int pn_metric_ssim(int C, int H, int W, const float* x, int64_t x_cs, int64_t x_ps, int x_tone, const float* y,
                   int64_t y_cs, int64_t y_ps, int y_tone, int window, const double* taps, double max_val, float* map,
                   double* out, double* work, void* stream);
/* [3, H, W] normal images; y goes through y_normalize passes of F.normalize first.  cos = F.cosine_similarity over the
 * channels (fp32, as ATen evaluates it), angle = nan_to_num(acos(cos)) in degrees (utils/metrics.py:240-257,
 * 368-397): out[5] = [sum angle, sum w angle, sum cos, sum w cos, count] */
int pn_metric_normals(int H, int W, const float* x, int64_t x_cs, int64_t x_ps, const float* y, int64_t y_cs,
                      int64_t y_ps, int y_normalize, double* out, double* work, void* stream);
/* depth metrics (utils/metrics.py:290-315) over n strided elements with mask > 0 (mask nullable: every element):
 * out[9] = [count, sum |d|/g, sum d^2/g, sum d^2, log count (also p, g > 1e-7), sum (log p - log g)^2,
 * then the counts of max(p/g, g/p) < 1.25, 1.25^2, 1.25^3] */
int pn_metric_depth(int64_t n, const float* pred, int64_t pred_st, const float* gt, int64_t gt_st, const float* mask,
                    int64_t mask_st, double* out, double* work, void* stream);

/* ---- geometry export: field queries and marching tetrahedra (pn_geometry.hip) -----------------------------------
 * Grid of nx x ny x nz vertices (every axis >= 2, nx ny nz < 2^31): vertex v = (i ny + j) nz + k sits at
 * (x0 + i dx, y0 + j dy, z0 + k dz), each coordinate evaluated in fp32 in exactly that form.  Cell (i, j, k),
 * i < nx - 1 etc., has index (i (ny - 1) + j)(nz - 1) + k.  A shape outside these bounds is PN_ERR_BAD_SHAPE. */
/* (mean, cov) rows [m, 3] of the vertices first .. first + m - 1; every axis of cov gets `variance` */
int pn_grid_points(int nx, int ny, int nz, int64_t first, int64_t m, float x0, float y0, float z0, float dx, float dy,
                   float dz, float variance, float* mean, float* cov, void* stream);
/* The activations of compute_graph (models/pano_mip_nerf.py:235-280) with the renderer's arithmetic, per row of
 * raw_rgb [M,3] / raw_density [M,nc] / grad_mean [M,3] (+ d sigma / d mean, as pn_chain_density_grad writes it).
 * Every output is nullable: sigma [M] = softplus(raw_0 + density_bias); albedo [M,3] = sigmoid(raw_1..3) 0.77 + 0.03
 * (nc = 5 only, PN_ERR_UNSUPPORTED otherwise); rgb [M,3] = softplus(raw_rgb) (1 + 2 rgb_padding) - rgb_padding;
 * normal [M,3] = -grad_mean / max(|grad_mean|, 1e-12).  sigma may point into a slab of a [nx, ny, nz] volume. */
int pn_field_epilogue(int64_t M, int num_density_channels, float density_bias, float rgb_padding, const float* raw_rgb,
                      const float* raw_density, const float* grad_mean, float* sigma, float* albedo, float* rgb,
                      float* normal, void* stream);
/* Marching tetrahedra of sigma [nx, ny, nz] (contiguous fp32) at `level`.
 *   inside <=> sigma > level (strict; NaN is outside).
 *   Each cell splits into 6 tetrahedra (Freudenthal / Kuhn): T0 = p, T1 = p + e_a, T2 = p + e_a + e_b, T3 = p + (1,1,1)
 *   for (a, b, c) = xyz, xzy, yxz, yzx, zxy, zyx in that order.  Every tetrahedron edge runs from a grid vertex u to
 *   u + o_s, o_s one of the 7 offsets s = 0 (1,0,0), 1 (0,1,0), 2 (0,0,1), 3 (1,1,0), 4 (1,0,1), 5 (0,1,1), 6 (1,1,1):
 *   neighbouring cells share every edge, so the mesh is watertight inside the grid.  Edge id = 7 u + s.
 *   Vertices [V,3]: one per edge whose endpoints differ in inside-ness, at p_u + t (p_b - p_u),
 *   t = (level - sigma_u) / (sigma_b - sigma_u), in ascending edge-id order.
 *   Faces [F,3] int32: by cell index, then tetrahedron, then the order of the case table below.
 *   Case table: case = in(T0) | in(T1) << 1 | in(T2) << 2 | in(T3) << 3; tetrahedron edges 0 (T0,T1), 1 (T0,T2),
 *   2 (T0,T3), 3 (T1,T2), 4 (T1,T3), 5 (T2,T3); triangles as edge triples for the even tetrahedra xyz, yzx, zxy:
 *     0: -            1: 012          2: 043          3: 124 143      4: 135          5: 052 035      6: 045 051
 *     7: 245          8: 254          9: 015 054     10: 053 025     11: 153         12: 134 142     13: 034
 *     14: 021         15: -
 *   (one lone vertex: its three edges; two and two, inside {a < b}, outside {c < d}: (ac, ad, bd), (ac, bd, bc)),
 *   wound so that (v1 - v0) x (v2 - v0) points to the outside (sigma <= level).  The odd tetrahedra xzy, yxz, zyx emit
 *   each triangle with its last two vertices swapped.
 * pn_mt_count: work = pn_mt_work_bytes(nx, ny, nz) bytes (device); writes totals[2] (device int64) = {V, F}.
 * pn_mt_emit: after pn_mt_count on the same sigma, level and work; num_vertices / num_faces are the rows of
 *   vertices / faces (the totals, copied by the caller); rows beyond them are not written.  Both must be < 2^31
 *   (PN_ERR_BAD_SHAPE otherwise).  Vertex coordinates use the placement of pn_grid_points.
 * Block sums, a scan of the block sums and a fix-up pass in separate launches: no atomics, the same output on every run. */
int64_t pn_mt_work_bytes(int nx, int ny, int nz);
int pn_mt_count(int nx, int ny, int nz, const float* sigma, float level, void* work, int64_t* totals, void* stream);
int pn_mt_emit(int nx, int ny, int nz, const float* sigma, float level, const void* work, int64_t num_vertices,
               int64_t num_faces, float x0, float y0, float z0, float dx, float dy, float dz, float* vertices,
               int32_t* faces, void* stream);

/* ---- spatially-varying lighting: light probes, SH and irradiance (pn_lighting.hip) ----------------------------
 * A light probe is an H x W equirectangular image (H, W >= 2) of HDR radiance.  Pixel pix = i W + j looks along the
 * viewdir pn_raygen_pano gives a camera with identity rotation (sample_dir_by_pano, utils/sampling.py:5-20; y up) and
 * covers the solid angle omega_i = sin((i + 1/2) pi / H) (2 pi / W) (pi / H) (solid_angle_refinement,
 * utils/surface_rendering.py:294-316).  That is upstream's unnormalised midpoint rule: its sum exceeds 4 pi by about
 * (pi / H)^2 / 24 relative (0.6 % at H = 8, 0.04 % at H = 32).  The caller passes the table: dirs [H W, 3], omega [H W].
 * Radiance of P probes is read at x[p * probe_stride + c * cs + pix * ps] (c = 0..2; strides in floats), so the
 * [P, 3, H, W] views of [P, H, W, 3] buffers are read in place.
 * SH: real, l <= 2, 9 coefficients per channel in the order (0,0) (1,-1) (1,0) (1,1) (2,-2) (2,-1) (2,0) (2,1) (2,2):
 * Y = 0.282095, 0.488603 {y, z, x}, 1.092548 {xy, yz}, 0.315392 (3 z^2 - 1), 1.092548 xz, 0.546274 (x^2 - y^2)
 * (constants to full double precision).  SH tensors are [., 9, 3] fp32 (coefficient-major, channel-minor).
 * Irradiance from SH (Ramamoorthi & Hanrahan 2001): E(n) = sum_lm A_l L_lm Y_lm(n), A = (pi, 2 pi / 3, pi / 4).
 * Every sum is fp64 in a fixed order, without atomics: repeated calls give the same bits.  NaN radiance propagates.
 * Errors: PN_ERR_BAD_SHAPE (P <= 0 or >= 2^25, H or W < 2, H W >= 2^30, K <= 0, a grid axis < 2). */
/* L_lm = sum_pix L(pix) Y_lm(dir_pix) omega_pix -> out [P, 9, 3]; work: pn_probe_sh_work_doubles(P, H, W) device
 * doubles of per-workgroup partial sums, added in order by a second launch */
int64_t pn_probe_sh_work_doubles(int64_t P, int H, int W);
int pn_probe_sh(int64_t P, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps,
                const float* dirs, const float* omega, float* out, double* work, void* stream);
/* exact quadrature E_p(n) = sum_pix L_p(pix) max(0, n . dir_pix) omega_pix (the shading of surface_rendering,
 * utils/surface_rendering.py:129-165, over every probe pixel) for normals [K, 3] shared by every probe
 * (per_probe_normals = 0) or [P, K, 3] (1) -> out [P, K, 3].  max as torch.relu: a NaN dot product stays NaN. */
int pn_probe_irradiance(int64_t P, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps,
                        const float* dirs, const float* omega, int64_t K, const float* normals, int per_probe_normals,
                        float* out, void* stream);
/* SH irradiance volume: sh [nx ny nz, 9, 3] at the vertices of a grid placed as by pn_grid_points (vertex
 * (i ny + j) nz + k at (x0 + i dx, ...)).  Per point of points [M, 3]: clamp it to the box, interpolate the 27
 * coefficients trilinearly, E(normal) with the A_l weights above -> out [M, 3] (normals [M, 3], unit length). */
int pn_sh_volume_irradiance(int nx, int ny, int nz, float x0, float y0, float z0, float dx, float dy, float dz,
                            const float* sh, int64_t M, const float* points, const float* normals, float* out,
                            void* stream);

/* ---- image-based lighting: GGX prefilter, environment-BRDF table, engine shading (pn_ibl.hip) -----------------------
 * The assets of the split-sum approximation (Karis, "Real Shading in Unreal Engine 4") from the light probes above (the
 * same probe addressing and the same dirs / omega tables).  Every sum is fp64 in a fixed order on fp32 inputs, rounded
 * once per output, without atomics: repeated calls give the same bits.
 * Prefilter (pn_prefilter): for directions [K, 3] shared by every probe (per_probe_directions = 0) or [P, K, 3] (1), unit
 * length, and alpha = roughness^2, roughness in (0, 1]: per probe pixel of direction d and solid angle omega
 *   c = max(0, n . d),  h2 = (1 + c) / 2 (= NoH^2 with N = V = R),  den = h2 (alpha^2 - 1) + 1,  q = c / den^2
 *   out[p, n, ch] = (sum (L_ch omega) q) / (sum omega q)  -> out [P, K, 3]
 * i.e. the GGX D NoL weights, the constant alpha^2 / pi of D cancelling.  A deterministic quadrature over every pixel, not
 * Monte Carlo.  The pixels are summed in index order within segments of consecutive LDS tiles and the segments in order;
 * the segmentation depends on H W only, so a probe's result does not depend on P.  work: pn_prefilter_work_doubles(P, H,
 * W, K) device doubles.  NaN as pn_probe_irradiance: a NaN radiance value makes its channel NaN for every direction of
 * the probe (weight 0 times NaN included), a NaN dot product stays NaN.  A zero direction gives 0 / 0 = NaN.
 * Table (pn_brdf_lut): out [size, size, 2] = (A, B) with specular = prefiltered (F0 A + B); row i has roughness r =
 * (i + 1/2) / size, column j NoV mu = (j + 1/2) / size.  N = z, V = (sqrt(1 - mu^2), 0, mu), alpha = r^2, k = alpha / 2;
 * midpoint rule on the GGX-warped grid u = (a + 1/2) / n, phi = 2 pi (b + 1/2) / n, a, b < n = samples:
 *   cos^2 theta_h = (1 - u) / (1 + (alpha^2 - 1) u),  H = (sin theta_h cos phi, sin theta_h sin phi, cos theta_h),
 *   VoH = V . H,  NoL = 2 VoH NoH - mu,  G1(x) = x / ((1 - k) x + k),  Gv = G1(NoL) G1(mu) VoH / (NoH mu),
 *   Fc = 2^(-(5.55473 VoH + 6.98316) VoH),  A = sum (1 - Fc) Gv / n^2,  B = sum Fc Gv / n^2   over NoL > 0 and VoH > 0.
 * One entry per wave: lane l adds the nodes a n + b = l, l + 64, ... in order, then a fixed butterfly.
 * Shading (pn_ibl_shade), one row per thread, for ONE probe's assets: specular_levels = the levels l < levels of the
 * prefiltered cube-map chain one after the other, level l a strip [3, 6 S_l, S_l], S_l = size >> l, holding roughness
 * l / (levels - 1); irradiance a strip [3, 6 Si, Si]; lut [St, St, 2].  viewdirs point from the camera to the surface.
 *   v = -viewdir / |viewdir|,  nv = n . v,  NoV = max(0, nv),  Rr = 2 nv n - v,  r = roughness[row] or roughness_all
 *   lambda = clamp(r (levels - 1), 0, levels - 1),  l0 = min(floor lambda, levels - 2),  f = lambda - l0
 *   light = (1 - f) fetch(level l0, Rr) + f fetch(level l0 + 1, Rr),  E = fetch(irradiance, n)
 *   fetch: the CUBE lookup of pn_reproject (face, s, t from the component of largest magnitude; bilinear around
 *     (px - 1/2, py - 1/2), the four taps clamped within the face, ((w00 v00 + w01 v01) + w10 v10) + w11 v11), in fp64;
 *     NaN for a zero or NaN direction.  No filtering across faces.
 *   (A, B) bilinear in lut at x = NoV St - 1/2 (columns), y = r St - 1/2 (rows), each clamped to [0, St - 1]
 *   diffuse = albedo / pi E,  specular = light (f0 A + B),  rgb = diffuse + specular (each rounded once from fp64)
 * Errors: PN_ERR_BAD_SHAPE (the probe limits of pn_probe_irradiance, K <= 0, roughness outside (0, 1], a table size < 2
 * or > 4096, samples < 1 or > 4096, levels < 2 or > 13 or size >> (levels - 1) < 1, a cube size < 1 or > 4096). */
int64_t pn_prefilter_work_doubles(int64_t P, int H, int W, int64_t K);
int pn_prefilter(int64_t P, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps, const float* dirs,
                 const float* omega, int64_t K, const float* directions, int per_probe_directions, double roughness,
                 float* out, double* work, void* stream);
int pn_brdf_lut(int size, int samples, float* out, void* stream);
int pn_ibl_shade(int64_t R, int size, int levels, const float* specular_levels, int irradiance_size,
                 const float* irradiance, int lut_size, const float* lut, const float* albedo, const float* normals,
                 const float* viewdirs, const float* roughness, float roughness_all, float f0, float* rgb, float* diffuse,
                 float* specular, void* stream);

/* ---- novel views: pinhole rays (pn_cameras.hip) and viewable frames (pn_views.hip) -------------------------------
 * Pinhole camera: pix2cam [3, 3] fp32 row-major maps pixel (x + 1/2, y + 1/2, 1) (x = column, y = row) to a camera-space
 * direction; the Blender form is ((x + 1/2 - W/2) / f, -(y + 1/2 - H/2) / f, -1): x right, y up, looking along -z
 * (datasets/base_datasets.py:216-265; Multicam passes its own pix2cam, :118-170).  Per ray, each product a 3-term fp32
 * dot product in index order: directions = c2w[:3,:3] @ (pix2cam @ p), NOT normalised; viewdirs = directions / |.|;
 * origins = c2w[:3, 3]; lossmult = 1; near / far as given; noise_var = 0; radii = |d(i, j) - d(i + 1, j)| 2 / sqrt(12)
 * with the NEXT ROW's direction (upstream's rule as written, although its comment says "x-axis neighbor"); row H - 1
 * reuses row H - 2's value.  Cameras: pix2cams [n_cam, 9], c2ws [n_cam, 16] (row-major 4x4), both device arrays.
 * Batch ray b is pixel idx[b] % (H W) of camera idx[b] / (H W) (an index outside the pool reads ray 0); rgb_pool
 * [n_cam H W, 3] and rgb_out [B, 3] are both given (target colours are gathered) or both NULL.
 * Errors: PN_ERR_BAD_SHAPE (B <= 0, n_cam <= 0, H or W < 2, H W >= 2^31). */
int pn_sample_pinhole_rays(int64_t B, int n_cam, int H, int W, const int64_t* idx, const float* pix2cams,
                           const float* c2ws, float near_, float far_, const float* rgb_pool, float* origins,
                           float* directions, float* viewdirs, float* radii, float* lossmult, float* near_out,
                           float* far_out, float* noise_var, float* rgb_out, void* stream);
/* Frames: one H x W image, element (c, pix) at x[c cs + pix ps] (strides in floats), -> out [H W, 3] uint8 (device),
 * the bytes systems/panonerf_system.py:77-131 writes through save_results (utils/vis.py:25-41): trunc(255 v), NaN -> 0.
 *   PN_FRAME_LDR     hdr_to_ldr(scale x, dtype='uint8'): k = trunc(255 clamp(aces)), v = (k / 255) ** (1 / 2.2)
 *   PN_FRAME_LDR_GT  hdr_to_ldr(scale x): v = clamp(aces) ** (1 / 2.2)
 *   PN_FRAME_DEPTH   hotmap((d - near) / range) (utils/vis.py:13-22): t = (d - near) / range, x = t - min / (max - min)
 *                    (upstream's precedence; min / max over the image, NaN-propagating), then matplotlib jet: i = trunc(256 x),
 *                    x == 1 -> 255, x < 0 -> lut[0], x > 1 -> lut[255], NaN -> black.  lut: [256, 3] fp32 (device);
 *                    work: 2 device floats (the min / max, written by a first single-workgroup launch)
 *   PN_FRAME_NORMAL  v = (x / max(|x|, 1e-12) + 1) / 2
 *   PN_FRAME_ALBEDO  v = clamp(x, 0, 1)
 * The tone mapping is pn_metrics.hip's (fp32, upstream's order of operations).  No atomics: repeated calls give the same
 * bytes.  Errors: PN_ERR_BAD_SHAPE (H or W <= 0, H W >= 2^31), PN_ERR_UNSUPPORTED (unknown kind). */
enum { PN_FRAME_LDR = 0, PN_FRAME_LDR_GT = 1, PN_FRAME_DEPTH = 2, PN_FRAME_NORMAL = 3, PN_FRAME_ALBEDO = 4 };
int pn_to_frame(int kind, int H, int W, const float* x, int64_t cs, int64_t ps, float scale, float near_, float range,
                const float* lut, float* work, uint8_t* out, void* stream);

/* ---- camera models and reprojection (pn_cameras.hip) ----------------------------------------------------------------
 * Camera space is the pinhole's: right-handed, x right, y up, looking along -z.  A camera is (kind, H, W, params): params
 * is a HOST array of PN_CAM_PARAMS floats, copied into the launch (unused entries are ignored).  Continuous pixel
 * positions put the centre of pixel (x = column, y = row) at (x + 1/2, y + 1/2).
 *   PN_CAM_PANO         the equirectangular camera of pn_raygen_pano: theta = -px 2 pi / W, phi = py pi / H,
 *                       d = (sin phi sin theta, cos phi, sin phi cos theta).  No params.  H >= 2, W >= 3.
 *   PN_CAM_PINHOLE      params[0..8] = pix2cam (d = pix2cam @ (px, py, 1), as pn_sample_pinhole_rays), params[9..17] =
 *                       cam2pix = inv(pix2cam), inverted in fp64 by the caller and rounded once.  H, W >= 2.
 *   PN_CAM_CUBE         a vertical strip of six S x S faces (W = S >= 2, H = 6 S) in the order +x, -x, +y, -y, +z, -z.
 *                       Within a face s = 2 px / S - 1, t = 2 (py - face S) / S - 1 (t points down) and
 *                         +x (1, -t, -s)   -x (-1, -t, s)   +y (s, 1, t)   -y (s, -1, -t)   +z (s, -t, 1)   -z (-s, -t, -1).
 *                       This is the OpenGL cube-map table, i.e. the LOOKUP convention engines use (direction -> face,
 *                       s, t): a face looked at as a picture is therefore mirrored relative to a pinhole view along the
 *                       same axis in this right-handed y-up world.  No params.
 *   PN_CAM_FISHEYE      equidistant: params[0] = f (pixels per radian, > 0), params[1] = theta_max (half the field of view,
 *                       radians, in (0, pi]).  u = px - W / 2, v = -(py - H / 2), r = hypot(u, v), theta = r / f,
 *                       d = (sin theta u / r, sin theta v / r, -cos theta), (0, 0, -1) at r = 0.  A position is inside the
 *                       image circle when theta <= theta_max.  H, W >= 2.
 *   PN_CAM_STEREO_PANO  one eye of an omnidirectional-stereo pair: params[0] = +ipd / 2 (right eye) or -ipd / 2 (left).
 *                       Directions are PN_CAM_PANO's; column j has the heading angle theta_j = -(j + 1/2) 2 pi / W and the
 *                       camera-space origin params[0] (-cos theta_j, 0, sin theta_j) = heading x up, so the ray is tangent
 *                       to the viewing circle.  Not a central projection: rays only.
 * Rays (pn_sample_camera_rays; kinds CUBE, FISHEYE, STEREO_PANO - the panorama and the pinhole keep their own entry points,
 * PN_ERR_UNSUPPORTED here): the contract of pn_sample_pinhole_rays - batch ray b is pixel idx[b] % (H W) of camera
 * idx[b] / (H W), an index outside the pool reads ray 0, rgb_pool / rgb_out both given or both NULL; every camera shares
 * (kind, H, W, params), c2ws [n_cam, 16] is a device array.
 *   CUBE, FISHEYE: directions = viewdirs = c2w[:3,:3] @ unit camera direction (3-term fp32 dot products in index order; the
 *     cube's table direction is divided by its fp32 norm first), origins = c2w[:3, 3], noise_var = 0, lossmult = 1,
 *     radii = |d(i, j) - d(i + 1, j)| 2 / sqrt(12) with the next row's direction, the last row reusing the one before (the
 *     pinhole rule); for the cube "row" is the row within the face.  A fisheye pixel outside the image circle gets the
 *     forward direction c2w[:3,:3] @ (0, 0, -1) and lossmult = 0; its radius still comes from the equidistant formula.
 *   STEREO_PANO: every field is pn_sample_pano_rays' except origins = c2w[:3,:3] @ offset + c2w[:3, 3]; with params[0] = 0
 *     the origin is c2w[:3, 3] itself and every field equals pn_sample_pano_rays' bit for bit (one device function).
 * Reprojection (pn_reproject; kinds PANO, PINHOLE, CUBE, FISHEYE on either side): image [N, C, Hs, Ws] with element
 * (n, c, pix) at image[n image_stride + c cs + pix ps] (strides in floats, so permuted views are read in place) ->
 * out [N, C, Hd, Wd] and coverage [Hd, Wd], both contiguous.  rotation_host: 3 x 3 row-major HOST matrix taking a
 * destination camera-space direction to a source camera-space direction (R_src_c2w^T R_dst_c2w for two posed cameras at
 * one position).  Per destination pixel (x, y) and subsample a, b < k = samples: position (x + (a + 1/2) / k,
 * y + (b + 1/2) / k) -> destination direction (invalid outside a fisheye's circle) -> rotated -> source position:
 *   PANO     phi = atan2(hypot(dx, dz), dy), theta = atan2(dx, dz), t = -theta / 2 pi, px = (t - floor t) W, py = phi H / pi;
 *            always valid.  Taps wrap in columns and clamp in rows.  At an exact pole theta = atan2(0, 0) = 0.
 *   PINHOLE  q = cam2pix @ d; valid iff q.z > 0 and (q.x, q.y) / q.z lies in [0, W] x [0, H].  Taps clamp to the edge.
 *   FISHEYE  theta = atan2(hypot(dx, dy), -dz), r = f theta, (px, py) = (W / 2 + r dx / rho, H / 2 - r dy / rho), rho =
 *            hypot(dx, dy) (the centre at rho = 0); valid iff theta <= theta_max and the position lies in [0, W] x [0, H].
 *            Taps clamp to the image.
 *   CUBE     the component of largest magnitude picks the face, ties going to the earlier face of the order above; with m
 *            that magnitude: +x (s, t) = (-dz, -dy) / m, -x (dz, -dy) / m, +y (dx, dz) / m, -y (dx, -dz) / m,
 *            +z (dx, -dy) / m, -z (-dx, -dy) / m; px = (s + 1) S / 2, py = (t + 1) S / 2 within the face.  Taps clamp
 *            within the face.
 * then the bilinear fetch around (px - 1/2, py - 1/2): ((w00 v00 + w01 v01) + w10 v10) + w11 v11 in fp32.  The output is
 * the sum of the valid subsamples' fetches in the order b outer, a inner, divided by their count; coverage is count / k^2;
 * with no valid subsample every channel gets `fill`.  NaN in the source propagates (a tap of weight 0 included).  No
 * atomics: repeated calls give the same bits.
 * Errors: PN_ERR_UNSUPPORTED (an unknown kind; a kind the entry point does not take), PN_ERR_BAD_SHAPE (B, n_cam, N or
 * C <= 0, a size below the kind's minimum, a cube with H != 6 W, H W >= 2^31, samples <= 0 or > PN_REPROJECT_MAX_SAMPLES,
 * fisheye params not positive). */
enum { PN_CAM_PANO = 0, PN_CAM_PINHOLE = 1, PN_CAM_CUBE = 2, PN_CAM_FISHEYE = 3, PN_CAM_STEREO_PANO = 4 };
#define PN_CAM_PARAMS 20
#define PN_REPROJECT_MAX_SAMPLES 16
int pn_sample_camera_rays(int64_t B, int n_cam, int kind, int H, int W, const float* params_host, const int64_t* idx,
                          const float* c2ws, float near_, float far_, const float* rgb_pool, float* origins,
                          float* directions, float* viewdirs, float* radii, float* lossmult, float* near_out,
                          float* far_out, float* noise_var, float* rgb_out, void* stream);
int pn_reproject(int N, int C, int src_kind, int Hs, int Ws, const float* src_params_host, int dst_kind, int Hd, int Wd,
                 const float* dst_params_host, const float* rotation_host, int samples, float fill, const float* image,
                 int64_t image_stride, int64_t cs, int64_t ps, float* out, float* coverage, void* stream);

/* ---- depth-aware view warping (pn_cameras.hip) ------------------------------------------------------------------------
 * Forward warping of RGB-D frames into other posed cameras with a z-buffer: pn_warp_splat scatters, pn_warp_resolve
 * gathers.  Cameras are the central kinds above (PANO, PINHOLE, CUBE, FISHEYE; STEREO_PANO is PN_ERR_UNSUPPORTED), params
 * HOST arrays as for pn_reproject; poses are device arrays of row-major 4x4 c2w (R = c2w[:3,:3], o = c2w[:3, 3]).  All S
 * sources share (src_kind, Hs, Ws, src_params), all D destinations (dst_kind, Hd, Wd, dst_params).  Everything is fp32,
 * separate operations in the order written (3-term sums associate to the left: (a + b) + c).
 * Splat, per source frame s < S and source pixel (i = row, j = column) with t = depth[s, i, j] (depth [S, Hs, Ws]):
 *   skip unless 0 < t < inf (NaN, 0, negative and Inf are no points).
 *   dc = the camera-space direction of the ray the samplers above give that pixel, i.e. at position (j + 1/2, i + 1/2):
 *     PANO unit (theta = -(j + 1/2) / W 2 pi, phi = (i + 1/2) / H pi, as pn_sample_pano_rays), PINHOLE pix2cam @ (px, py, 1)
 *     NOT normalised, CUBE the table direction divided by its norm, FISHEYE unit; a fisheye pixel with theta > theta_max
 *     is skipped.  So t is the distance along that sampler's ray (the renderer's depth output) for every camera.
 *     |dc| = sqrt((x x + y y) + z z) for a pinhole and exactly 1 for the others.
 *   X = (R_s dc) t + o_s  (R_s dc by 3-term dot products in index order, then one product and one sum per component).
 * then per destination d < D:
 *   e = R_d^T (X - o_d)  (e_k = (R[0][k] v_0 + R[1][k] v_1) + R[2][k] v_2),  rho = sqrt((e_0 e_0 + e_1 e_1) + e_2 e_2);
 *   skip unless 0 < rho < inf.
 *   (qx, qy, face) = the position of direction e in the destination camera by the inverse projections of pn_reproject (qy
 *   within the face for a cube); skip where that is invalid (behind or off a pinhole's frame, outside a fisheye's circle).
 *   Footprint: a(i, j) = |u(y, j) - u(y + 1, j)| with u the UNIT direction of a pixel centre (the equidistant formula
 *   also outside a fisheye's circle; PANO here by theta = -(px / W) 2 pi, phi = (py / H) pi) and the row rule of the radii
 *   above: rows count within a cube's face, y = min(row, rows - 2).  a_s = a(i, j) of the source camera; a_d that of the
 *   destination camera at the landing pixel (min(max(floor qy, 0), rows - 1), min(max(floor qx, 0), W - 1)) of `face`.
 *     size = (scale ((t |dc|) a_s)) / (rho a_d):  the angular size of the source pixel seen from the destination, in
 *     destination pixels, times scale.   k = 1 unless size > 1 (a NaN size too); else min(max_splat, ceil(size)).
 *   Pixels: columns x0 .. x0 + k - 1 with x0 = floor(qx - (k - 1) / 2), rows y0 .. y0 + k - 1 with y0 = floor(qy - (k - 1) / 2).
 *   A destination panorama's columns wrap; every other column and every row outside the image (a cube: outside the face)
 *   is dropped.  A fisheye is not clipped to its circle.
 *   For each pixel (y, x): zbuf[d, y, x] = min(zbuf[d, y, x], (uint64(bits of rho) << 32) | (s Hs Ws + i Ws + j)), a 64-bit
 *   unsigned atomic minimum.  rho > 0, so its bits order as its value; the low word makes every key unique (ties in rho go
 *   to the lower source index), so the result does not depend on the order of the atomics: repeated calls give the same
 *   bits.  zbuf [D, Hd, Wd] uint64 is set to all ones (PN_WARP_EMPTY) by the caller; several splats may share one zbuf.
 * Resolve, per destination d and pixel: key = zbuf[d, y, x].  Empty (all ones, or a low word >= S Hs Ws): index = -1,
 * depth_out = NaN, coverage = 0 and every channel = fill.  Otherwise index = the low word (int64), coverage = 1,
 * depth_out = rho / |d_dst| with d_dst the destination's ray direction at the pixel centre (|d_dst| = |pix2cam @ (x + 1/2,
 * y + 1/2, 1)| for a pinhole, no division for the others): again the distance along that camera's ray.  out[d, c, y, x] =
 * image[s image_stride + c cs + pix ps] of that source pixel (image [S, C, Hs, Ws] addressed as in pn_reproject; NaN
 * propagates).  image and out may both be NULL: depth, index and coverage only.  out [D, C, Hd, Wd], depth_out, index
 * (int64) and coverage [D, Hd, Wd] are contiguous.  One launch each on `stream`; no workspace.
 * Errors: PN_ERR_UNSUPPORTED (an unknown kind, STEREO_PANO), PN_ERR_BAD_SHAPE (S or D <= 0, a size below the kind's
 * minimum, S Hs Ws >= 2^32, D Hd Wd >= 2^31, max_splat outside [1, PN_WARP_MAX_SPLAT], scale not positive and finite,
 * fisheye params not positive, C <= 0 with an image), PN_ERR_NULL (a required pointer; image without out or the reverse). */
#define PN_WARP_MAX_SPLAT 8
#define PN_WARP_EMPTY 0xffffffffffffffffull
int pn_warp_splat(int S, int src_kind, int Hs, int Ws, const float* src_params_host, const float* depth,
                  const float* src_c2ws, int D, int dst_kind, int Hd, int Wd, const float* dst_params_host,
                  const float* dst_c2ws, int max_splat, float scale, uint64_t* zbuf, void* stream);
int pn_warp_resolve(int S, int C, int Hs, int Ws, int D, int dst_kind, int Hd, int Wd, const float* dst_params_host,
                    const uint64_t* zbuf, const float* image, int64_t image_stride, int64_t cs, int64_t ps, float fill,
                    float* out, float* depth_out, int64_t* index, float* coverage, void* stream);

/* ---- finishing warped frames: "the same surface", blending and hole filling (pn_cameras.hip, pn_inpaint.hip) --------------
 * One parameter depth_ratio = r in [0, 1) decides whether two depths belong to one surface: positive depths a <= b do iff
 * b (1 - r) <= a.  q = 1 - r is one fp32 subtraction on the host; every comparison costs one fp32 product.  Everything is
 * fp32, separate operations in the order written; sums associate to the left and start from their first term.  The usual
 * r = 0.05 is a convention, not a measurement.
 *
 * Blending (pn_warp_blend): S layers of D warped frames, images [S, D, C, H, W], depths [S, D, H, W], weights [S, D] (a
 * DEVICE array; positive and finite, which the caller checks), all contiguous.  Per destination d and pixel:
 *   a layer s counts iff 0 < z_s < inf (z_s = depths[s, d, pixel]; NaN, 0, negative and Inf are no points).
 *   No layer counts: every channel = fill, depth_out = NaN, coverage = 0.
 *   Otherwise zn = the smallest such z_s; the layers with z_s q <= zn are kept, the others are occluded.  coverage = 1.
 *   One layer kept: its colours and its depth are copied, bit for bit.
 *   Several kept: (sum of w_s v_s) / (sum of w_s) over the kept layers in layer order, for each colour and for z
 *   (w_s = weights[s, d]; NaN in a kept colour propagates).
 * out [D, C, H, W], depth_out and coverage [D, H, W] are contiguous.  One launch, one thread per pixel, gathers only.
 * Errors: PN_ERR_BAD_SHAPE (a size <= 0, r outside [0, 1) or not finite, S D C H W >= 2^31), PN_ERR_NULL (any pointer).
 *
 * Hole filling (pn_fill_holes): push-pull over a pyramid that fills a hole from its FARTHER neighbours only - a
 * disocclusion shows what lay behind the foreground, so the foreground must not bleed into it.  In place on N images:
 * image [N, C, H, W], depth [N, H, W] or NULL, known [N, H, W] fp32 (known iff > 0) or NULL (all known), domain [H, W]
 * uint8 shared by all images or NULL (all inside), filled [N, H, W] uint8 (written everywhere).  A pixel is known iff it
 * is inside the domain, its `known` is > 0 and, with a depth, 0 < z < inf; its z is depth's, or 1 without a depth (plain
 * push-pull).  A pixel outside the domain is never known and never written.
 * Levels: level 0 is the frame; level l is ((H_{l-1} + 1) >> 1) x ((W_{l-1} + 1) >> 1); the pyramid has L levels above
 * the frame: up to 1 x 1, or `levels` if that is fewer (PN_FILL_ALL_LEVELS: up to 1 x 1).  A texel holds C colours and z;
 * z = 0 is unknown.
 * Pull, l = 1 .. L, per texel (y, x) of level l: its children (2 y + dy, 2 x + dx) in the order (0,0), (0,1), (1,0), (1,1)
 * that exist in level l - 1 and are known.  None: the texel is unknown.  Otherwise zf = their largest z, the children
 * with zf q <= z_i are kept, and each colour and z is the sum over the kept children in that order divided by their
 * count (as a float).
 * Push, l = L - 1 .. 0, after level l + 1's own push; only the unknown texels of level l (at level 0: inside the domain)
 * are written.  Four taps in level l + 1: rows (near, far) = ((y - 1) >> 1, (y + 1) >> 1) for odd y and (y / 2, y / 2 - 1)
 * for even y, columns by the same rule on x; in the order and with the weights (near, near) 9, (near row, far column) 3,
 * (far row, near column) 3, (far, far) 1.  Rows clamp to the level; columns clamp too, or with wrap_x (a panorama) wrap
 * modulo W_{l+1}; a clamped duplicate counts twice.  The known taps: none, and the texel stays unknown.  Otherwise zf =
 * their largest z, the taps with zf q <= z_i are kept, and each colour and z is (sum of w_i v_i) / (sum of w_i) over the
 * kept taps in tap order.
 * Outputs: the holes of image (and depth) are filled, known pixels keep their bits; filled = 1 where a value was written
 * and 0 elsewhere; a pixel no level reaches (capped levels, nothing known) keeps its input bits.  A NaN colour of a known
 * pixel propagates into what it fills.
 * One call makes every launch on `stream` (at most 2 L, a pull and a push per level; the levels of at most 1024 texels
 * share one launch, one workgroup per image with their planes in LDS: the same arithmetic, the same bits): one thread
 * per texel looping over the channels, gathers only, no atomics, no host read or synchronisation, so repeated calls
 * give the same bits.  work holds
 * levels 1 .. L as [N, C + 1, H_l, W_l] planes: pn_fill_holes_work_floats(N, C, H, W, levels) floats (work_floats is what
 * the caller has; with L = 0 nothing is needed and work may be NULL).
 * Errors: PN_ERR_BAD_SHAPE (a size <= 0, N (C + 1) H W >= 2^31, r outside [0, 1) or not finite, levels < 0, work_floats too
 * small; pn_fill_holes_work_floats returns it as its value), PN_ERR_NULL (image, filled, or work with L > 0). */
#define PN_FILL_ALL_LEVELS 32
int pn_warp_blend(int S, int D, int C, int H, int W, const float* images, const float* depths, const float* weights,
                  float depth_ratio, float fill, float* out, float* depth_out, float* coverage, void* stream);
int64_t pn_fill_holes_work_floats(int N, int C, int H, int W, int levels);
int pn_fill_holes(int N, int C, int H, int W, float* image, float* depth, const float* known, const uint8_t* domain,
                  int wrap_x, float depth_ratio, int levels, uint8_t* filled, float* work, int64_t work_floats,
                  void* stream);

/* ---- dataset ingest (pn_data.hip) ---------------------------------------------------------------------------------
 * planes: the channel planes of one decoded scanline OpenEXR file as stored, [Hs][n_ch][Ws] (line, channel, column),
 * fp16 (is_half != 0) or fp32, on the device.  out: [Hs / factor, Ws / factor, C] fp32 interleaved, C = 1 for
 * PN_INGEST_DEPTH and 3 otherwise.  Output channel k reads plane c0 / c1 / c2 (R, G, B by plane index; depth reads c0 only).
 * Each output value is the mean of its factor x factor source block (cv2.resize INTER_AREA at an integer factor that
 * divides both sides; datasets/pano_datasets.py:76-78): HALF widened to fp32, ONE fp32 accumulator per channel over rows
 * then columns in index order, divided by factor^2 - a fixed order, so repeated calls give the same bits.  Then the
 * fix-up of datasets/pano_datasets.py:100-116:
 *   PN_INGEST_IMAGE   NaN -> 0, then clip to [0, 1000]
 *   PN_INGEST_ALBEDO  none
 *   PN_INGEST_NORMAL  x * 2 - 1; flag != 0 (pano scenes): x and z negated (the right product with R_y(pi))
 *   PN_INGEST_DEPTH   flag != 0 (normalize_depth): clip(d, near, far) (NaN stays NaN), then (d - near) / (far - near)
 * One launch on `stream`; no workspace, no atomics.  Errors: PN_ERR_BAD_SHAPE (a size <= 0, factor does not divide Hs
 * and Ws, Hs Ws n_ch >= 2^31, a plane index outside [0, n_ch), far <= near with normalised depth),
 * PN_ERR_UNSUPPORTED (unknown kind). */
enum { PN_INGEST_IMAGE = 0, PN_INGEST_ALBEDO = 1, PN_INGEST_NORMAL = 2, PN_INGEST_DEPTH = 3 };
int pn_ingest_image(int Hs, int Ws, int n_ch, int is_half, const void* planes, int c0, int c1, int c2, int factor, int kind,
                    int flag, float near_, float far_, float* out, void* stream);

/* ---- virtual object insertion: mesh tracing, probe shading, shadows (pn_objects.hip) ----------------------------------
 * Triangles: pn_tri_setup turns vertices [V, 3] + faces [F, 3] int32 into tris [F, 12] fp32 rows (v0, 0, e1 = v1 - v0, 0,
 * e2 = v2 - v0, 0), once per mesh; a face with an index outside [0, V) becomes the all-zero triangle, which nothing hits.
 * bsphere: 4 device floats (centre, radius) of a sphere that holds every vertex, or NULL (pn_trace_mesh only): rays and
 * points that cannot reach it (tested in fp64 with the radius widened by 0.1 % + 1e-6) skip the triangles; the results do
 * not depend on it.
 * Ray / triangle test (primary and shadow rays alike): Moeller-Trumbore in fp32, separate operations in this order:
 * p = d x e2, det = e1 . p, inv = 1 / det, s = o - v0, u = (s . p) inv, q = s x e1, v = (d . q) inv, t = (e2 . q) inv.
 * Edge rule: a hit needs det != 0, u >= -eps, v >= -eps, u + v <= 1 + eps (all inclusive, eps = PN_OBJ_EDGE_EPS: two
 * triangles that share an edge both own a band of 2e-6 barycentric units around it, so fp32 rounding opens no gap in
 * a closed mesh; u and v are reported as computed, so they may lie that far outside [0, 1]) and 0 < t < +inf (exclusive),
 * t < t_max[r] (exclusive) where t_max is given.  Two-sided: the sign of det is not looked at.  Directions are NOT
 * normalised: t is in units of d, as the renderer's `distance`.  hit = (1 - u - v) v0 + u v1 + v v2.
 * Tie-break: faces are visited in index order and a face replaces the best so far only when its t is smaller, so among
 * equal t the lowest face index wins, whatever the tile size.  A miss: t = +inf, face = -1, bary = 0.
 * Shading (pn_shade): surface_rendering (utils/surface_rendering.py:129-165) with the probe's pixels as the lights:
 * env = probe radiance, l = the probe directions, solid_angle = omega (the tables of the lighting section), and
 * v = -viewdirs: viewdirs are camera-to-surface unit vectors (what the renderer calls viewdirs) and the BRDF wants the
 * direction TOWARDS the eye.  K probes [K, 3, H, W] (1 <= K <= PN_OBJ_MAX_PROBES) are blended per row with weights
 * [R, K] (NULL with K = 1: weight 1): the light of row r is sum_k weights[r, k] L_k(pix) (surface_rendering_wlit,
 * :168-203; shading is linear in the light).  microfacet = 0: shading = sum L relu(n . l) omega, diffuse = albedo / pi
 * shading, specular = 0.  microfacet = 1: microfeast_brdf (:6-61) term for term - h = normalize(l + v), NoH, VoH, NoL,
 * NoV clamped at 0, alpha = r^2, k = r^2 / 2, D = alpha^2 / (pi (NoH^2 (alpha^2 - 1) + 1)^2), F = 0.04 + 0.96
 * 2^(-(5.55473 VoH + 6.98316) VoH), G = NoL / ((1 - k) NoL + k) NoV / ((1 - k) NoV + k), spec = D F G / (4 NoL NoV) with
 * NaN and +inf -> 0; diffuse = albedo / pi sum L NoL omega, specular = sum spec L omega (no NoL), shading not written
 * (pass NULL).  roughness: [R] or NULL (then roughness_all for every row).  rgb = fl(diffuse) + fl(specular).  All of it
 * in fp64 on the fp32 inputs, pixels in order, rounded once per output.
 * Shadow (pn_shadow_ratio): for scene point x with unit normal n under ONE probe [3, H, W]: E(S) = sum_{pix in S}
 * mean_c L_c(pix) max(0, n . l_pix) omega_pix; ratio = E(unoccluded) / E(all) clamped to [0, 1], where pix is occluded
 * when the ray from fl(x + fl(bias n)) along l_pix hits a triangle (the test above, t > 0, no t_max).  Only pixels with
 * n . l_pix > 0 are traced.  ratio = 1 when E(all) is not > 0, when x or n is not finite, and when F = 0.
 * Hit attributes (pn_object_hits), per ray: mask = (0 <= face < F) and not (t >= scene_dep) (scene_dep NULL: every hit;
 * a NaN depth counts as behind); for a masked ray points = o + t d, normals = the barycentric blend of vertex_normals
 * (or, NULL, normalize(e1 x e2)) renormalised and negated when n . d > 0 (i.e. n . v < 0), albedo = the blend of
 * vertex_albedo (or, NULL, the constant colour), viewdirs = d / |d|, weights [R, K] = 1 / |point - probe_positions[k]|
 * normalised to sum 1 (a position within 1e-6 takes its probe alone; weights may be NULL); zeros for the other rays.
 * scene_points (optional; needs scene_dep) = o + scene_dep d outside the mask, NaN inside.  fp64 on fp32 inputs, rounded once.
 * Composite (pn_object_composite): rgb = mask ? object_rgb : scene_rgb * shadow, depth = mask ? t : scene_dep.
 * No atomics anywhere; sums in pixel order: repeated calls give the same bits, whatever R.  R = 0 launches nothing.
 * Errors: PN_ERR_BAD_SHAPE (a negative count, F = 0 in pn_trace_mesh, K outside [1, 8], H or W < 2, H W >= 2^30). */
#define PN_OBJ_MAX_PROBES 8
#define PN_OBJ_EDGE_EPS 2e-6f
int pn_tri_setup(int64_t F, int64_t V, const float* vertices, const int32_t* faces, float* tris, void* stream);
/* any_hit = 0: t [R], face [R], bary [R, 2] are written (hit unused); any_hit = 1: hit [R] uint8 only */
int pn_trace_mesh(int64_t R, const float* origins, const float* directions, int64_t F, const float* tris,
                  const float* t_max, const float* bsphere, int any_hit, float* t, int32_t* face, float* bary,
                  uint8_t* hit, void* stream);
int pn_shade(int64_t R, int K, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps,
             const float* dirs, const float* omega, const float* albedo, const float* normals, const float* viewdirs,
             const float* roughness, float roughness_all, int microfacet, const float* weights, float* rgb,
             float* diffuse, float* specular, float* shading, void* stream);
int pn_shadow_ratio(int64_t R, int H, int W, const float* x, int64_t cs, int64_t ps, const float* dirs,
                    const float* omega, const float* points, const float* normals, float bias, int64_t F,
                    const float* tris, const float* bsphere, float* out, void* stream);
int pn_object_hits(int64_t R, const float* origins, const float* directions, const float* t, const int32_t* face,
                   const float* bary, const float* scene_dep, int64_t V, const float* vertices, int64_t F,
                   const int32_t* faces, const float* vertex_normals, const float* vertex_albedo, float albedo_r,
                   float albedo_g, float albedo_b, int K, const float* probe_positions, uint8_t* mask, float* points,
                   float* normals, float* albedo, float* viewdirs, float* weights, float* scene_points, void* stream);
int pn_object_composite(int64_t R, const uint8_t* mask, const float* object_rgb, const float* t,
                        const float* scene_rgb, const float* scene_dep, const float* shadow, float* rgb, float* depth,
                        void* stream);

/* ---- mesh tracing through a device-built BVH (built by pn_bvh.hip, walked by pn_bvh_walk.h for pn_tri.h's BvhFinder): opt-in
 * The ray / triangle test is the one above (the same function, on the same tris rows).  A BVH skips triangles whose box
 * the ray misses, and the fp32 test above is not exact (it owns a band of PN_OBJ_EDGE_EPS outside each triangle and its t
 * is badly conditioned for grazing rays), so a BVH cannot promise the brute-force result for every input.  It promises a
 * result that does not depend on the tree, and that is the brute-force result wherever no accepted (ray, triangle) pair
 * falls outside the triangle's padded box:
 * Triangle box of face f: lo / hi = the fp32 component-wise min / max of its three vertices (the vertices themselves,
 * not v0 + e1), widened on every side by pad = fl(fl(PN_BVH_PAD_REL * ext) + fl(PN_BVH_PAD_ABS * mag)), ext = the largest
 * of the three fl(hi - lo), mag = the largest |coordinate| of the three vertices: box = [fl(lo - pad), fl(hi + pad)].
 * A face with an index outside [0, V) or a vertex coordinate that is not finite gets the EMPTY box (lo = +inf,
 * hi = -inf), which no ray passes: such a face is never a candidate.
 * Box test of ray (o, d): a ray with a component of o or d that is not finite passes nothing (the test above never
 * accepts such a ray either); a box with lo.x > hi.x (empty) is passed by nothing.  Otherwise per axis, fp32, separate
 * operations, inv = 1 / d: when inv is finite, a = fl(fl(lo - o) inv), b = fl(fl(hi - o) inv), near = min(a, b), far =
 * max(a, b); when it is not (d == 0, or so small that 1 / d overflows) the axis is a slab: near = -inf, far = +inf when
 * lo <= o <= hi, else the box is missed - so no 0 x inf is ever formed and no NaN decides anything.  tn = the largest near,
 * tf = the smallest far, both then rounded outwards: tn (1 - 2^-21) for tn > 0, tn (1 + 2^-21) otherwise; tf (1 + 2^-21)
 * for tf > 0, tf (1 - 2^-21) otherwise.  The box is passed when tn <= tf and tf >= 0.
 * Candidate rule: face f counts for ray r iff the test above accepts it (t < t_max[r] exclusive included), the ray
 * passes f's own padded box, and tn_f <= t_f.  Closest hit: the lexicographic minimum of (t, f) over the candidates
 * (equal t: the lowest face index).  any_hit and shadow occlusion: the candidate set is not empty.
 * The tree cannot matter: a node's box is the exact fp32 union (min / max, no arithmetic) of its children's boxes, down
 * to the padded triangle boxes; fp32 subtraction, multiplication by a fixed inv, min / max, the slab branch and the
 * outward rounding are all monotone, so a parent's tn is never above a child's and its tf never below.  A traversal skips
 * a node only when the ray does not pass its box or tn_node > best (strict; best starts at t_max or +inf); a leaf's t
 * replaces the best when t < best, or t == best with a face already held and f lower.  Hence every ancestor of the
 * winning candidate is entered whatever the topology and the order of traversal.
 * The constants: the edge band lies at most 2e-6 (|e1| + |e2|) <= 7e-6 ext outside the triangle, and fp32 rounding moves
 * the point o + t d that the test accepts by a few ulp of the coordinates involved; PAD_REL = 1e-4 covers the band 14
 * times over and PAD_ABS = 4e-6 is 64 ulp of the triangle's largest coordinate; the slab arithmetic's own relative error
 * (2 roundings, 2^-23) sits inside the outward rounding of 2^-21.  With them no accepted pair of the test scenes
 * (tests/test_bvh_cpu.py: closed, random, sliver, coincident and fan meshes under panoramic, pinhole, vertex- and
 * edge-aimed, axis-aligned and inside-the-box rays) fails the candidate rule, so there BVH == brute force bit for bit;
 * with no padding the same test counts 14 accepted pairs outside their boxes.  The pad knows the triangle only: an eye
 * whose distance dwarfs the mesh's coordinates is outside what the constants were sized for.
 * Build (all on `stream`, no host synchronisation): pn_bvh_boxes writes tbox [F, 2, 4] = (lo, 0), (hi, 0) per face;
 * the caller takes their union (scene_box: 6 device floats lo, hi) and pn_bvh_keys writes one 63-bit Morton key per
 * face (21 bits per axis of the box centre within scene_box, x the most significant of each triple; int64 >= 0; an empty
 * box: 2^63 - 1); the caller sorts them (stable) into sorted_keys and order (order[j] = the face at sorted position j);
 * pn_bvh_tree builds the radix tree of Karras (2012) over the sorted keys, one thread per internal node, equal keys told
 * apart by their sorted position, and refits bottom-up: one thread per leaf climbs, the second arrival at a node (an
 * atomicAdd on counters behind a fence) goes on with the union.  Min / max are exact, so the nodes do not depend on the
 * arrival order: two builds give the same bytes.
 * nodes [max(F - 1, 1), 16] fp32, row i = (lo_left, ref_left), (hi_left, ref_right), (lo_right, parent), (hi_right, 0):
 * both children's boxes in one 64-byte row; ref, parent: int32 bits; ref >= 0 an internal node, ref < 0 the leaf of face
 * ~ref, PN_BVH_NONE no child; the root is row 0 with parent -1.  F = 1: no internal node is built; row 0 carries the one
 * leaf as its left child and (empty box, PN_BVH_NONE) on the right.
 * Depth: the split position of a node is a common-prefix length of (key, sorted position) pairs, it grows strictly from
 * parent to child, and it takes at most PN_BVH_KEY_BITS + 31 values (F < 2^31): no leaf lies under more than
 * PN_BVH_MAX_DEPTH = 94 internal nodes, and a traversal that pushes at most one child per level holds at most that many.
 * Work: leaf_parent [F] int32 and counters [max(F - 1, 1)] int32 (zeroed by pn_bvh_tree itself).
 * pn_trace_mesh_bvh / pn_shadow_ratio_bvh: the outputs and conventions of pn_trace_mesh / pn_shadow_ratio with the
 * candidate rule above; the shadow's sums, their order and its horizon / bounding-sphere early-outs are unchanged, so its
 * ratio has the brute-force bits whenever the occlusion booleans agree.  The traversal stack lives in LDS.
 * Errors: PN_ERR_BAD_SHAPE (a negative count, F <= 0 or F >= 2^31 where a tree is needed). */
#define PN_BVH_PAD_REL 1e-4f
#define PN_BVH_PAD_ABS 4e-6f
#define PN_BVH_KEY_BITS 63
#define PN_BVH_MAX_DEPTH 94
#define PN_BVH_NONE (-2147483647 - 1)
int pn_bvh_boxes(int64_t F, int64_t V, const float* vertices, const int32_t* faces, float* tbox, void* stream);
int pn_bvh_keys(int64_t F, const float* tbox, const float* scene_box, int64_t* keys, void* stream);
int pn_bvh_tree(int64_t F, const int64_t* sorted_keys, const int64_t* order, const float* tbox, float* nodes,
                int32_t* leaf_parent, int32_t* counters, void* stream);
int pn_trace_mesh_bvh(int64_t R, const float* origins, const float* directions, int64_t F, const float* tris,
                      const float* nodes, const float* t_max, int any_hit, float* t, int32_t* face, float* bary,
                      uint8_t* hit, void* stream);
int pn_shadow_ratio_bvh(int64_t R, int H, int W, const float* x, int64_t cs, int64_t ps, const float* dirs,
                        const float* omega, const float* points, const float* normals, float bias, int64_t F,
                        const float* tris, const float* nodes, const float* bsphere, float* out, void* stream);

/* ---- texture-mapped materials for inserted objects (pn_textures.hip): runs after pn_object_hits, which is untouched ------
 * Storage: a texture of H x W texels (1 <= H, W <= PN_TEX_MAX_SIZE) is one fp32 device buffer of float4 texels (16-byte
 * aligned), all mip levels concatenated: level l has h_l = max(1, H >> l) rows of w_l = max(1, W >> l) texels, row-major,
 * L = 1 + floor(log2(max(H, W))) levels, level 0 first.  pn_tex_floats(H, W) = 4 sum_l h_l w_l is the size in floats.
 * pn_tex_ingest writes level 0 from a device image [H, W, C] (1 <= C <= 4), uint8 (is_u8 != 0) or fp32: channels past C
 * are 0 and alpha (channel 3) is 1.  A uint8 channel 0 .. 2 is table[byte] (256 device floats the caller built: i / 255
 * or the sRGB EOTF, rounded once from fp64), a uint8 alpha is fl(i / 255); fp32 is copied.
 * pn_tex_pyramid fills levels 1 .. L-1 on `stream`, one launch per level: texel (y, x) of level l+1 is
 * ((a + b) + (c + d)) * 0.25f in fp32, a = (r0, c0), b = (r0, c1), c = (r1, c0), d = (r1, c1) of level l with rows
 * r0 = min(2y, h_l - 1), r1 = min(2y + 1, h_l - 1) and columns c0 = min(2x, w_l - 1), c1 = min(2x + 1, w_l - 1).
 * pn_texture_hits, per row r of the outputs of pn_object_hits (mask, and the face, bary, directions, t it was given;
 * normals_in = its shading normals, already flipped towards the eye), with uv [T, 2] and face_uv [F, 3] int32 (NULL: the
 * UVs are per vertex and indexed by faces), radii [R] or NULL, and up to three textures (NULL: no such map) - albedo,
 * roughness (channel 0) and a tangent-space normal map: writes albedo [R, 3], roughness [R], normals [R, 3] (normals may
 * alias normals_in) and, when not NULL, lod [R, 3] = the level of detail used per texture (0 for a NULL one).  An output
 * whose texture is NULL is not touched and may be NULL.  Rows outside the mask (or whose face / vertex index is out of
 * range) get zeros.  For a masked row, all in fp64 on the fp32 inputs, rounded once per output:
 *   UV: (U, V) = w0 uv0 + u uv1 + v uv2, (u, v) = bary, w0 = 1 - u - v.  A non-finite U or V gives sample 0; a face_uv
 *     index outside [0, T) reads as a non-finite UV.
 *   Footprint (ray cone; Akenine-Moeller et al., Ray Tracing Gems ch. 20): e1 = v1 - v0, e2 = v2 - v0, A_w = |e1 x e2|,
 *     A_uv = |du1 dv2 - du2 dv1| (du_i = u_i - u_0, ...), c = |n_g . d| / |d| with n_g = (e1 x e2) / A_w, width = 2 radii[r]
 *     t[r] (the renderer's cone radius at o + t d is t radii; radii NULL: width 0).  Per texture
 *     lambda = 0.5 log2(W H A_uv / A_w) + log2(width) - log2(c), clamped to [0, L - 1], NaN -> 0: a zero footprint samples
 *     level 0 and a grazing ray the top level; no epsilon is involved.
 *   Bilinear at level l: x = U w_l - 0.5, y = (flip_v ? 1 - V : V) h_l - 0.5, x0 = floor(x), fx = x - x0 (likewise y); the
 *     indices x0, x0 + 1 are wrapped by a non-negative modulo (wrap = 0, repeat) or clamped to [0, w_l - 1] (wrap = 1);
 *     value = (1 - fy) ((1 - fx) a00 + fx a01) + fy ((1 - fx) a10 + fx a11).
 *   Trilinear: l0 = floor(lambda), f = lambda - l0, l1 = min(l0 + 1, L - 1), out = (1 - f) s(l0) + f s(l1) (f == 0 reads
 *     level l0 only).  Roughness is channel 0, unclamped.
 *   Normal map: m = 2 s - 1, det = du1 dv2 - du2 dv1, T = (e1 dv2 - e2 dv1) / det, B = (e2 du1 - e1 du2) / det, N =
 *     normals_in[r]; T' = normalize(T - N (N . T)), B' = normalize(B - N (N . B) - T' (T' . B)) (Gram-Schmidt, no cross
 *     product: the handedness follows the UVs), n = normalize(m.x T' + m.y B' + m.z N).  The output is N, bit for bit,
 *     when det == 0, when a norm before normalising is < 1e-12, when anything is non-finite (a non-finite UV included),
 *     or when n . d >= 0 (the perturbed normal faces away from the eye).
 * One thread per row or texel, no LDS, no atomics: repeated calls give the same bits, whatever R.  R = 0 launches nothing.
 * Errors: PN_ERR_BAD_SHAPE (a size outside [1, PN_TEX_MAX_SIZE], C outside [1, 4], a negative count, wrap not 0 or 1),
 * PN_ERR_NULL (a required pointer, or the output of a texture that is given). */
#define PN_TEX_MAX_SIZE 16384
int64_t pn_tex_floats(int H, int W);
int pn_tex_ingest(int H, int W, int C, int is_u8, const void* image, const float* table, float* tex, void* stream);
int pn_tex_pyramid(int H, int W, float* tex, void* stream);
int pn_texture_hits(int64_t R, const uint8_t* mask, const int32_t* face, const float* bary, const float* directions,
                    const float* t, const float* normals_in, const float* radii, int64_t V, const float* vertices,
                    int64_t F, const int32_t* faces, int64_t T, const float* uv, const int32_t* face_uv,
                    const float* albedo_tex, int albedo_h, int albedo_w, const float* roughness_tex, int roughness_h,
                    int roughness_w, const float* normal_tex, int normal_h, int normal_w, int wrap, int flip_v,
                    float* albedo, float* roughness, float* normals, float* lod, void* stream);

/* ---- baking the scene into a texture atlas (pn_atlas.hip): one patch per face, read back by pn_texture_hits --------------
 * Layout: a square atlas of S x S texels (1 <= S <= PN_TEX_MAX_SIZE) is cut into cells of c x c texels
 * (PN_ATLAS_MIN_CELL <= c <= S), n = S / c (integer division) per row; texels with a row or column >= n c belong to
 * nobody.  Cell k = row n + col holds face 2k in its lower-left half (h = 0) and face 2k + 1 in its upper-right half
 * (h = 1); F <= 2 n^2.  With x along columns and y along rows, texel (li, lj) of a cell has its centre at (lj + 0.5,
 * li + 0.5), and the corners of face f, in continuous texel coordinates of its cell, are (L = c - 2 PN_ATLAS_MARGIN -
 * PN_ATLAS_DIAG = c - 4, the leg)
 *     h = 0:  P0 = (1, 1)          P1 = (1 + L, 1)          P2 = (1, 1 + L)
 *     h = 1:  P0 = (c - 1, c - 1)  P1 = (c - 1 - L, c - 1)  P2 = (c - 1, c - 1 - L)
 * corner Pi for vertex i of the face: a margin of PN_ATLAS_MARGIN texel to the cell's border, and PN_ATLAS_DIAG texels
 * between the two hypotenuses.
 * pn_atlas_uv writes uv [3F, 2] (row 3f + i: corner i of face f; face_uv[f] = (3f, 3f + 1, 3f + 2)) in the OBJ convention
 * pn_texture_hits reads with flip_v = 1: U = X / S, V = 1 - Y / S, (X, Y) = (col c, row c) + Pi, in fp64, rounded once.
 * Ownership of texel (li, lj) of cell k: h = (li + lj + 1 >= c), f = 2k + h; unowned when f >= F.  Its barycentrics are
 * those of the texel's centre (x, y) in the face's affine map - h = 0: u = (x - 1) / L, v = (y - 1) / L; h = 1:
 * u = (c - 1 - x) / L, v = (c - 1 - y) / L - extrapolated outside the triangle, never clamped: a gutter texel carries the
 * continuation of its own triangle's plane, so no dilation pass is needed.
 * Tap property (c >= 6): at any point of the closed UV triangle of a face, every level-0 bilinear tap of pn_texture_hits
 * (x = U S - 0.5, ...) with a non-zero weight is a texel that face owns.  A tap's centre is within one texel of the
 * sample in x and in y, so it stays inside the cell (margin 1); on triangle 0 the sample has x + y <= c - 2, its taps'
 * centres x + y <= c, with equality only for the far tap of a sample at integer x - 0.5 and y - 0.5, whose weight is 0:
 * every other tap has li + lj + 1 < c.  Triangle 1 mirrors it: x + y >= c + 2 and every tap has li + lj + 1 >= c.
 * Mip levels above 0 mix neighbouring cells, as with every per-triangle atlas: a baked asset is sampled at level 0 (radii
 * NULL) or re-atlased by the engine.
 * pn_atlas_texels, per texel t = i S + j of the image (fp64 on the fp32 inputs, rounded once per output): face [S, S]
 * int32 (-1: unowned), bary [S, S, 2] = (u, v), points [S, S, 3] = w0 v0 + u v1 + v v2 (w0 = 1 - u - v), normals_g =
 * (e1 x e2) / A_w (e1 = v1 - v0, e2 = v2 - v0, A_w = |e1 x e2|), normals_s = the barycentric blend of vertex_normals
 * divided by max(its norm, 1e-30) as pn_object_hits defines it, NOT flipped (normals_g when vertex_normals is NULL), and
 * var [S, S] = A_w / (12 L^2): the face's world area over its L^2 / 2 texels is the area of a texel's footprint, and a
 * square of that area has this second moment per axis.  Unowned texels get zeros in every float output; so do the texels
 * of a face with an index outside [0, V) or a non-finite vertex coordinate (face keeps f).  A face with A_w == 0 keeps
 * face, bary and points; its normals (both) and var are 0.
 * pn_atlas_encode_normals, per texel: (0.5, 0.5, 1) where face is outside [0, F); otherwise 0.5 m + 0.5 with m = (n . T',
 * n . B', n . N), n = world_normals[t], N = normals_s[t] and T', B' the Gram-Schmidt frame of pn_texture_hits built
 * from the face's edges and uv rows 3f .. 3f + 2 (as pn_atlas_uv wrote them) - the same expressions, so the sampler's
 * n = normalize(m.x T' + m.y B' + m.z N) returns the baked normal.  (0.5, 0.5, 1) also where that frame does not exist
 * (det == 0, a norm < 1e-12, anything non-finite, a vertex index outside [0, V)) or n . N <= 0: the sampler decodes it
 * to N bit for bit.
 * pn_atlas_quantize: x [count, C] fp32 (1 <= C <= 4) -> uint8.  With table (256 device floats, increasing, table[0] = 0:
 * the decode table of pn_tex_ingest) the code i whose table[i] is nearest to clamp(x, 0, 1), compared in fp64, the lower
 * code on a tie; without, round-half-even(255 clamp(x, 0, 1)).  NaN gives 0.
 * One face / texel / value per thread, no LDS, no atomics: repeated calls give the same bits.  F = 0 or count = 0 launch
 * nothing in pn_atlas_uv / pn_atlas_quantize.
 * Errors: PN_ERR_BAD_SHAPE (S or c outside their range, F < 0 or F > 2 n^2, V < 0, C outside [1, 4]), PN_ERR_NULL. */
#define PN_ATLAS_MARGIN 1
#define PN_ATLAS_DIAG 2
#define PN_ATLAS_MIN_CELL 6
int pn_atlas_uv(int64_t F, int S, int c, float* uv, void* stream);
int pn_atlas_texels(int S, int c, int64_t F, int64_t V, const float* vertices, const int32_t* faces,
                    const float* vertex_normals, int32_t* face, float* bary, float* points, float* normals_g,
                    float* normals_s, float* var, void* stream);
int pn_atlas_encode_normals(int S, int c, int64_t F, int64_t V, const float* vertices, const int32_t* faces,
                            const float* uv, const int32_t* face, const float* normals_s, const float* world_normals,
                            float* out, void* stream);
int pn_atlas_quantize(int64_t count, int C, const float* x, const float* table, uint8_t* out, void* stream);

/* ---- relighting: virtual point and spot lights with omnidirectional shadow maps (pn_relight.hip) ----------------------
 * Rows are rays with what the renderer found along them, so every camera works (the stereo panorama included):
 * origins, directions [R, 3] as the ray generators give them (directions NOT normalised), depth [R] = t along that ray
 * (the renderer's `distance`), normals [R, 3] or NULL, albedo and rgb [R, 3] (both, or neither when only visibility is
 * wanted).  Lights: L device rows of PN_LIGHT_FLOATS = 16 floats: position p (0-2), RGB radiant intensity I (3-5), spot
 * axis (6-8; all zero: an omni light; taken as given, pass a unit vector), cos_inner (9), cos_outer (10), r_min (11),
 * reserved zeros (12-15).  Shadow maps: maps [L, Hm, Wm] fp32, one per light, of kind PN_CAM_PANO (Hm, Wm >= 2) or
 * PN_CAM_CUBE (Hm = 6 Wm): the picture an identity-rotation camera of that kind at p takes of the EUCLIDEAN distance to
 * the nearest surface along each pixel's unit ray.  Outputs, each optional: out [R, 3], direct [R, 3], visibility [R, L].
 * Everything below is fp64 on the fp32 inputs (the scalars are fp32 too), operations in the written order, dot products
 * (a0 b0 + a1 b1) + a2 b2, every output rounded once (as pn_shade).
 * Row: valid iff 0 < t < +inf and, with normals, n finite and |n| > 1e-12; then n^ = n / |n| (n^ = 0 without normals).
 *   X = o + t d.
 * Light l, in index order:  w = p - X, r2 = w . w; the light contributes nothing (V = 0) unless r2 > 0.
 *   l = w / sqrt(r2);  NoL = max(0, n^ . l), or 1 without normals;
 *   s = clamp(((-(l . axis)) - cos_outer) / (cos_inner - cos_outer), 0, 1), spot = (s s) (3 - 2 s), or 1 for a zero axis;
 *   g = NoL spot.  If g is not > 0 (NaN included): V = 0 and no texel is read.
 * Visibility: Y = X + normal_offset n^, v = Y - p, rho = |v|; V = 0 unless 0 < rho < +inf.
 *   (qx, qy, face) = the position of direction v by pn_reproject's inverse projection, in fp64: PANO phi = atan2(hypot(vx,
 *   vz), vy), theta = atan2(vx, vz), u = -theta / (2 pi), qx = (u - floor u) Wm, qy = phi / pi Hm; CUBE the table of that
 *   section with S = Wm (cube_pos of pn_rays.h), qy within the face.
 *   tan = min(sqrt(max(0, 1 - NoL NoL)) / NoL, 10);  delta = pi / Hm (PANO) or 2 / Wm (CUBE): the angular size of a texel;
 *   slope = ((((bias_slope rho) delta) tan) (k + 1)) / 2, or 0 without normals;  k = pcf, odd, <= PN_RELIGHT_MAX_PCF.
 *   Samples: for b < k (outer), a < k (inner): position (qx + (a - (k - 1) / 2), qy + (b - (k - 1) / 2)), and around
 *   (x - 1/2, y - 1/2) the four bilinear taps of pn_reproject's rule: x0 = floor, x1 = x0 + 1, weights wx = the fraction;
 *   a panorama's columns wrap and its rows clamp (so at a pole the window repeats the last row, and does not cross to the
 *   opposite meridian), a cube's taps clamp within the face (nothing is filtered across a seam).
 *   Tap with texel z: dark (c = 0) iff z is finite, z > 0 and rho > ((z (1 + bias_rel)) + bias_abs) + slope; else c = 1:
 *   a NaN, Inf, zero or negative texel is "no surface" and lights.
 *   Sample = ((w00 c00 + w01 c01) + w10 c10) + w11 c11, w00 = (1 - wy)(1 - wx), w01 = (1 - wy) wx, w10 = wy (1 - wx),
 *   w11 = wy wx;  V = (the samples summed in that order) / (k k).
 * Shading: where V > 0, E_c = E_c + ((I_c g) V) / max(r2, r_min r_min) (a light with V = 0 adds nothing);
 *   direct_c = (albedo_c / pi) E_c: Lambert, the convention of pn_shade's diffuse = albedo / pi shading, with I in radiance
 *   units x length^2 (radiant intensity: a light of intensity I at distance r facing the surface gives E = I / r^2);
 *   out_c = fl(ambient rgb_c + direct_c), visibility[r, l] = fl(V).
 * An invalid row: direct = 0, V = 0 for every light, out = fl(ambient rgb).  L = 0 is legal: out = fl(ambient rgb).
 * One row per thread, the lights in index order, no atomics: repeated calls give the same bits, whatever R and however
 * the rows are split over calls.  R = 0 launches nothing.
 * Errors: PN_ERR_BAD_SHAPE (R or L < 0, pcf even or outside [1, PN_RELIGHT_MAX_PCF], a non-finite scalar, a negative
 * bias_abs / bias_rel / bias_slope, Hm or Wm < 2, Hm Wm >= 2^31, a cube with Hm != 6 Wm), PN_ERR_UNSUPPORTED (a map kind
 * other than PANO and CUBE), PN_ERR_NULL (origins, directions or depth; lights or maps with L > 0; albedo or rgb missing
 * while out or direct is wanted). */
#define PN_LIGHT_FLOATS 16
#define PN_RELIGHT_MAX_PCF 7
int pn_relight(int64_t R, const float* origins, const float* directions, const float* depth, const float* normals,
               const float* albedo, const float* rgb, int L, const float* lights, int map_kind, int Hm, int Wm,
               const float* maps, float ambient, float normal_offset, float bias_abs, float bias_rel, float bias_slope,
               int pcf, float* out, float* direct, float* visibility, void* stream);

/* ---- emitters: the light sources of an HDR probe as connected bright regions with their radiometry (pn_emitters.hip) ----
 * Probes are read as pn_probe_sh reads them: x[p * probe_stride + c * cs + pix * ps], pix = i W + j row-major over an
 * H x W equirectangular image, H, W >= 2; dirs [H W, 3] and omega [H W] are the table of the lighting section.
 * Luminance: Y = ((double)R + G + B) / 3.0, the mean pn_shadow_ratio uses for a probe pixel.
 * Emitter pixel: Y > threshold[p], strict and in fp64; a NaN Y (or a NaN threshold) is no emitter, Y = +inf is one.
 * Default threshold (pn_emitter_threshold): fl(ratio exp(sum_pix omega ln max(Y, 1e-6) / sum_pix omega)), the sums over the
 *   pixels with finite Y, in fp64: ratio times the solid-angle-weighted GEOMETRIC mean, because the arithmetic mean of a
 *   probe is dominated by the very lamps it is meant to find.  The rule and the usual ratio of 8 are conventions, not
 *   measurements.  One workgroup of 1024 threads per probe; thread t adds pixels t, t + 1024, ... in order, then a fixed tree.  A probe
 *   with no finite pixel gets NaN: nothing in it is an emitter.
 * Adjacency: the 8-neighbourhood with column W - 1 next to column 0, the diagonals across that seam included ((i, 0) touches
 *   (i + 1, W - 1)); rows 0 and H - 1 are NOT joined across the poles.
 * Labels: int32 [P, H, W], -1 for background; the components of a probe are numbered 0 .. C - 1 in ascending order of
 *   their smallest pixel index, which fixes the result whatever the schedule.  Three calls:
 *   pn_emitter_labels   label equivalence (union-find over pixel indices; 32-bit atomicMin on parent, so the surviving root
 *                       of a component is its smallest pixel index): parent [P H W] is workspace, roots [P, H, W] gets
 *                       every pixel's root index within its probe (-1 background), flags [P, H, W] gets 1 at a root, else 0
 *   (the caller)        prefix = the inclusive running count of flags along each probe, int32 [P, H W]
 *   pn_emitter_compact  labels (on entry: roots) becomes prefix[root] - 1 in place, count[p] = prefix[p, H W - 1]
 * Record of component c of probe p (pn_emitter_stats), row s = p Cmax + c of every output; all sums in fp64 on the fp32
 *   inputs, each output rounded once.  The caller passes the pixels grouped by component: order [N] int64 holds global
 *   pixel indices p H W + pix, and starts [P Cmax + 1] int64 the offsets of the rows in it, so that order[starts[s] ..
 *   starts[s + 1]) are the pixels of row s in ascending order (a stable sort by label).  One wave per row: lane l adds
 *   elements l, l + 64, ... in order and the lanes meet in the xor butterfly 32, 16, .., 1: a fixed order, no floating-point
 *   atomics, the same bits on every call.  The work is proportional to the pixels listed plus the rows, not to C x H W.
 *     pixels          the number of pixels
 *     omega           sum omega_pix
 *     flux [3]        sum L_c omega_pix
 *     lum_flux        sum Y omega_pix
 *     direction [3]   normalize(sum Y omega_pix d_pix); where that sum's norm is below 1e-12 lum_flux (or is zero or not
 *                     finite) the direction of the peak pixel
 *     peak, peak_index   the largest Y and its pixel index, the lowest index among ties
 *     spread          the largest angle atan2(|direction x d_pix|, direction . d_pix) over the component's pixels
 *     angular_radius  acos(1 - min(omega, 4 pi) / (2 pi)): the cap of equal solid angle
 *     distance        sum Y omega dist / sum Y omega over the pixels with 0 < dist < +inf of distance [P, H W] (contiguous);
 *                     NaN with no such pixel or with distance = NULL
 *   A row with starts[s] = starts[s + 1] is not written: zero the outputs first.  Entries of order that are not pixels of
 *   the row's probe are skipped.
 * The light a component stands for, in pn_relight's units: position = probe position + direction distance, radius =
 *   distance sin(min(angular_radius, pi / 2)), intensity[3] = flux distance^2: a point light of that intensity adds `flux`
 *   to the irradiance of a surface at the probe that faces it, which is what the component adds in pn_probe_irradiance up
 *   to sum lum_flux 2 sin(spread / 2) (|relu(n . d) - relu(n . u)| <= |d - u|).
 * Errors: PN_ERR_BAD_SHAPE (P <= 0 or >= 2^25, H or W < 2, H W >= 2^30, P H W >= 2^39, a ratio that is not finite and
 * positive, Cmax < 0 or > H W, N < 0 or > P H W), PN_ERR_NULL (any pointer but `distance`; `order` may be null with N = 0).
 * Cmax = 0 launches nothing. */
int pn_emitter_threshold(int64_t P, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps,
                         const float* omega, double ratio, float* threshold, void* stream);
int pn_emitter_labels(int64_t P, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps,
                      const float* threshold, int32_t* parent, int32_t* roots, int32_t* flags, void* stream);
int pn_emitter_compact(int64_t P, int H, int W, const int32_t* prefix, int32_t* labels, int32_t* count, void* stream);
int pn_emitter_stats(int64_t P, int H, int W, const float* x, int64_t probe_stride, int64_t cs, int64_t ps,
                     const float* dirs, const float* omega, const float* distance, int Cmax, int64_t N,
                     const int64_t* order, const int64_t* starts, int32_t* pixels, float* omega_out, float* flux,
                     float* lum_flux, float* direction, float* peak, int32_t* peak_index, float* spread,
                     float* angular_radius, float* distance_out, void* stream);

/* ---- TSDF fusion: posed depth images integrated into a truncated signed distance volume (pn_fusion.hip) -----------------
 * Grid: pn_grid_points' grid (every axis >= 2, nx ny nz < 2^31), vertex v = (i ny + j) nz + k; tsdf and weight are
 * contiguous fp32 [nx, ny, nz], read and written in place.  weight = 0 marks a voxel no view has seen: the caller zeroes
 * weight for a fresh volume, and where weight is 0 the content of tsdf is ignored on input.
 * Views: S depth images of ONE central camera (kind, H, W, params; PANO, PINHOLE, CUBE or FISHEYE as in the camera section,
 * params a HOST array as for pn_reproject; STEREO_PANO is PN_ERR_UNSUPPORTED) at the poses c2ws, a device array [S, 16] of
 * row-major c2w (R = c2w[:3,:3], o = c2w[:3, 3]).  depth [S, H, W] is the distance t along the ray the samplers give each
 * pixel, exactly what pn_warp_splat reads (the renderer's depth output; for a pinhole that ray is not normalised).
 * confidence [S, H, W] or NULL, view_weights device [S] or NULL.
 * Everything below is fp64 on the fp32 inputs (the scalars are fp32 too and are widened first), operations in the written
 * order, dot products (a0 b0 + a1 b1) + a2 b2, every output rounded once (as pn_relight).
 * Voxel (i, j, k):  X = (x0 + i dx, y0 + j dy, z0 + k dz);  A = B = 0.  Then for each view s in index order:
 *   1. v = X - o_s,  e_k = (R[0][k] v_0 + R[1][k] v_1) + R[2][k] v_2  (e = R_s^T v),  rho = sqrt((e_0 e_0 + e_1 e_1) + e_2 e_2);
 *      skip the view unless 0 < rho < +inf.
 *   2. (qx, qy, face) = the position of direction e by pn_reproject's inverse projection, in fp64, with its validity rules:
 *      PANO     phi = atan2(hypot(e_x, e_z), e_y), theta = atan2(e_x, e_z), u = -theta / (2 pi), qx = (u - floor u) W,
 *               qy = phi / pi H; always valid.
 *      PINHOLE  q = cam2pix @ e (params[9..17], row by row); valid iff q_z > 0 and (qx, qy) = (q_x, q_y) / q_z lies in
 *               [0, W] x [0, H].
 *      FISHEYE  r = hypot(e_x, e_y), theta = atan2(r, -e_z); valid iff theta <= theta_max and (qx, qy) = (W / 2 + (f theta)
 *               e_x / r, H / 2 - (f theta) e_y / r) (the centre at r = 0) lies in [0, W] x [0, H].
 *      CUBE     the table of the camera section with S = W (cube_pos of pn_rays.h), qy within the face; always valid.
 *      Skip the view where that is invalid.
 *   3. The NEAREST pixel: column min(max(floor qx, 0), W - 1), row min(max(floor qy, 0), rows - 1) with rows = H, or rows = W
 *      and the row counted within `face` for a cube.  Depth is not interpolated: a bilinear fetch across a depth
 *      discontinuity invents a surface between foreground and background that no view saw.
 *   4. t = depth[s, row, column];  skip unless 0 < t < +inf and t <= depth_max (NaN, 0, negative and Inf are no surface).
 *   5. w = view_weights[s] (1 if NULL), times confidence[s, row, column] if given;  skip unless 0 < w < +inf.
 *   6. z = t |dc|, dc the camera-space direction of that pixel's centre as pn_warp_splat defines it: for a PINHOLE
 *      c_k = (p[3k] (column + 1/2) + p[3k + 1] (row + 1/2)) + p[3k + 2] of pix2cam and |dc| = sqrt((c_0 c_0 + c_1 c_1) + c_2 c_2);
 *      exactly 1 for the other kinds (z = t).  So z is the Euclidean distance of the surface that pixel saw.
 *   7. sdf = z - rho: the signed distance along the voxel's own ray (positive in front of the surface).  Skip if
 *      sdf < -trunc: the voxel is behind the surface and unseen from this view.
 *   8. d = min(1, sdf / trunc);  A = A + w d,  B = B + w.
 * After the views: if B == 0 the voxel keeps its bits (tsdf and weight).  Otherwise, with W0 = weight[v] and D0 = tsdf[v]
 * (D0 = 0 if W0 == 0):  W1 = W0 + B,  tsdf[v] = fl((D0 W0 + A) / W1),  weight[v] = fl(min(W1, max_weight)): the weighted
 * running mean of the usual TSDF fusion, with the weight capped so that later views can still move an old volume.
 * One voxel per thread, the views in index order inside the kernel, A and B in registers, no atomics: repeated calls give
 * the same bits, whatever the launch geometry.  One launch takes all S views, so nothing carries between launches; two
 * calls over views [0, a) and [a, S) round tsdf and weight to fp32 in between and are NOT the one call over [0, S).
 * Errors: PN_ERR_UNSUPPORTED (an unknown kind, STEREO_PANO), PN_ERR_BAD_SHAPE (a grid axis < 2, nx ny nz >= 2^31, S <= 0, a
 * size below the kind's minimum, a cube with H != 6 W, S H W >= 2^31, trunc not positive and finite, depth_max or
 * max_weight not > 0 (+inf is allowed), fisheye params not positive), PN_ERR_NULL (params_host, c2ws, depth, tsdf, weight). */
int pn_tsdf_integrate(int nx, int ny, int nz, float x0, float y0, float z0, float dx, float dy, float dz, int S, int kind,
                      int H, int W, const float* params_host, const float* c2ws, const float* depth, const float* confidence,
                      const float* view_weights, float trunc, float depth_max, float max_weight, float* tsdf, float* weight,
                      void* stream);

/* ---- mesh operations: connected components and quadric vertex clustering of triangle meshes (pn_meshops.hip) -----------
 * A mesh is vertices [V, 3] fp32 and faces [F, 3] int32, both contiguous, V and F < 2^31.  Every kernel checks the indices
 * it reads: a face with a corner outside [0, V) takes no part anywhere (pn_mesh_check reports it so that the caller can
 * raise first).  Sorts, scans and compactions are the caller's; everything that computes is here.  All floating-point
 * work is fp64 on the fp32 inputs, operations in the written order (dot products (a0 b0 + a1 b1) + a2 b2, cross products
 * (u1 w2 - u2 w1, u2 w0 - u0 w2, u0 w1 - u1 w0)), each output rounded once; no floating-point atomics; the same bits on
 * every call.
 *
 * pn_mesh_check: bad[0] = 1 if a coordinate is not finite, bad[1] = 1 if a face index is outside [0, V); else 0.
 *   vertices may be NULL: then only the faces are judged.
 *
 * Components.  Two faces are connected if they share a vertex INDEX.  Union-find over vertex indices (pn_unionfind.h, the
 * loop of the emitters; termination: DESIGN.md 6j): a vertex some face uses starts as its own parent, every other vertex
 * as -1; one thread per face unites v0-v1 and v1-v2 with 32-bit atomicMin, so the root of a component is its smallest
 * vertex index whatever the schedule.  Three steps:
 *   pn_mesh_components  parent [V] is workspace; roots [V] gets every vertex's root (-1: no face uses it), flags [V] 1 at a root
 *   (the caller)        prefix = the inclusive running count of flags, int32 [V]
 *   pn_mesh_labels      vertex_label [V] = prefix[root] - 1 (-1 for an unused vertex), face_label [F] = the label of the
 *                       face's first corner, count[0] = prefix[V - 1]: labels 0 .. C - 1 in ascending order of the root
 * pn_mesh_component_stats: the record of every component.  The caller passes the faces grouped by label: order [F] int64
 *   (a STABLE sort of the face indices by face_label) and starts [C + 1] int64, so that order[starts[c] .. starts[c + 1])
 *   are the faces of component c in ascending index.  That list is cut into chunks of 4096: chunk j holds its elements
 *   [4096 j, 4096 (j + 1)).  chunk_starts [C + 1] int64 is the running count of ceil(n_c / 4096), from 0; B >= chunk_starts[C]
 *   is the number of workgroups launched (F / 4096 + C bounds it without a host copy) and work holds 10 B doubles.
 *   One workgroup of 256 threads per chunk: thread t adds elements t, t + 256, ... of the chunk in order, starting from
 *   0.0; the 64 lanes of a wave meet in the xor butterfly 32, 16, .., 1; thread 0 adds waves 0, 1, 2, 3 in order.  Then one
 *   thread per component adds its chunks' sums in ascending j, sequentially, from 0.0.  The work is one visit of every face
 *   plus one workgroup per chunk and one thread per component, not
 *   C x F.  With n = (b - a) x (c - a) of a face (a, b, c):
 *     nfaces    the number of faces                      nverts   the number of vertices with that label (integer atomics)
 *     area      fl((sum sqrt((n0 n0 + n1 n1) + n2 n2)) / 2)
 *     volume    fl((sum (a0 x0 + a1 x1) + a2 x2) / 6) with x = b x c: the signed volume, positive for outward winding
 *     bbox [6]  min x, y, z then max x, y, z over the faces' corners (fp32, exact)
 *   All five outputs must be zeroed by the caller; a component without a valid face is not written.
 *
 * Quadric vertex clustering (Lindstrom 2000 on Rossignac-Borrel cells).
 *   Cells: lo is fp32 per axis, cell one fp32 scalar > 0, n per axis >= 1.  The cell index of a coordinate v on an axis is
 *     floor((double(v) - double(lo)) / double(cell)) clamped to [0, n - 1] (the clamp in fp64), and the key of a vertex is
 *     (ix ny + iy) nz + iz, int64 (nx ny nz must fit 63 bits).  pn_cluster_keys writes keys [V].  A cluster is an occupied
 *     cell; clusters are ordered by ascending key (the caller sorts the keys STABLY, takes the unique ones - cluster_keys [K]
 *     - and with them rank [V] int32, vertex_order [V] = the vertices grouped by cluster in ascending index, and
 *     vertex_starts [K + 1]).
 *   Faces (pn_cluster_faces, K < 2^21): out_faces [F, 3] = rank of each corner, winding and corner order kept; face_keys
 *     [F] = (s0 << 42) | (s1 << 21) | s2 of the sorted triple s0 < s1 < s2, or 2^63 - 1 where two corners are equal (the
 *     face is dropped).  Faces of equal key have the same unordered vertex set, whatever their winding: the caller keeps
 *     the lowest face index of each key (a stable sort), survivors in their original order.
 *   Solve (pn_cluster_solve), ONE THREAD PER CLUSTER, everything sequential.  With c = the cell centre,
 *     c_a = double(lo_a) + (double(i_a) + 0.5) double(cell):
 *     1. for the vertices v of the cluster in ascending index (vertex_order[vertex_starts[k] .. vertex_starts[k + 1])):
 *        m += double(v) - c per axis, and the sums of the rows of normals and colors (where given); cnt counts them.
 *        xbar = m / cnt.  out_normals = the mean g / cnt divided by its norm sqrt((g0 g0 + g1 g1) + g2 g2), or 0 where that
 *        norm is below 1e-12; out_colors = the mean.
 *     2. for the incidences i = 3 f + corner whose corner's vertex lies in the cluster, in ascending i (incidence_order
 *        [3 F] = a stable sort of i by the cluster rank of faces[i], incidence_starts [K + 1]): with the face (a, b, c_),
 *        u = b - a, w = c_ - a, n = u x w (unnormalised: weights of area squared, no sqrt), d = -((n0 (a0 - c0) + n1 (a1 - c1))
 *        + n2 (a2 - c2)):  A00 += n0 n0, A01 += n0 n1, A02 += n0 n2, A11 += n1 n1, A12 += n1 n2, A22 += n2 n2, b_k += n_k d.
 *        A face with two corners in the cluster is added twice; a zero-area face adds zeros.
 *     3. t = (A00 + A11) + A22.  If t == 0: x = xbar, flags = 2.  Otherwise s = lam t, q_kk = A_kk + s, r_k = s xbar_k - b_k,
 *        and LDL^T with + - * / only:
 *          l10 = A01 / q00, l20 = A02 / q00, d1 = q11 - l10 A01, u12 = A12 - l20 A01, l21 = u12 / d1,
 *          d2 = (q22 - l20 A02) - l21 u12, y1 = r1 - l10 r0, y2 = (r2 - l20 r0) - l21 y1,
 *          x2 = y2 / d2, x1 = y1 / d1 - l21 x2, x0 = (r0 / q00 - l10 x1) - l20 x2.
 *        x is accepted (flags = 0) iff every component is finite and |x_k| <= double(cell) 0.5; otherwise x = xbar and
 *        flags = 1 (Lindstrom's fallback).  lam (1e-3 by convention) makes the system SPD with a condition number of
 *        about 1 / lam: a flat or creased cluster is pulled to xbar along its free directions only.
 *     4. out_vertices[k] = fl(c + x) per axis.
 * Errors: PN_ERR_BAD_SHAPE (V or F negative or >= 2^31, C or K outside [0, V], B negative, K >= 2^21 in pn_cluster_faces, lo or cell not
 * finite, cell <= 0, n < 1, nx ny nz beyond 63 bits, lam negative or not finite), PN_ERR_NULL (a required pointer; normals
 * and colors and their outputs are optional, but an output needs its input).  V = 0, C = 0, K = 0 launch nothing. */
int pn_mesh_check(int64_t V, int64_t F, const float* vertices, const int32_t* faces, int32_t* bad, void* stream);
int pn_mesh_components(int64_t V, int64_t F, const int32_t* faces, int32_t* parent, int32_t* roots, int32_t* flags,
                       void* stream);
int pn_mesh_labels(int64_t V, int64_t F, const int32_t* faces, const int32_t* roots, const int32_t* prefix,
                   int32_t* vertex_label, int32_t* face_label, int32_t* count, void* stream);
int pn_mesh_component_stats(int64_t V, int64_t F, int64_t C, const float* vertices, const int32_t* faces,
                            const int64_t* order, const int64_t* starts, const int64_t* chunk_starts, int64_t B,
                            double* work, const int32_t* vertex_label, int32_t* nfaces, int32_t* nverts, float* area,
                            float* volume, float* bbox, void* stream);
int pn_cluster_keys(int64_t V, const float* vertices, float lox, float loy, float loz, float cell, int64_t nx, int64_t ny,
                    int64_t nz, int64_t* keys, void* stream);
int pn_cluster_faces(int64_t F, int64_t V, int64_t K, const int32_t* faces, const int32_t* rank, int32_t* out_faces,
                     int64_t* face_keys, void* stream);
int pn_cluster_solve(int64_t K, int64_t V, int64_t F, const float* vertices, const int32_t* faces, const float* normals,
                     const float* colors, float lox, float loy, float loz, float cell, int64_t nx, int64_t ny, int64_t nz,
                     const int64_t* cluster_keys, const int64_t* vertex_order, const int64_t* vertex_starts,
                     const int64_t* incidence_order, const int64_t* incidence_starts, double lam, float* out_vertices,
                     float* out_normals, float* out_colors, uint8_t* flags, void* stream);

/* ---- mesh distance: the closest point of a triangle mesh to arbitrary points, and surface sampling (pn_meshdist.hip) -----
 * A mesh is vertices [V, 3] fp32 and faces [F, 3] int32, contiguous, V and F < 2^31; points [P, 3] fp32.  Everything is
 * fp64 on the fp32 inputs, separate operations in the written order (dot (a0 b0 + a1 b1) + a2 b2; cross (u1 w2 - u2 w1,
 * u2 w0 - u0 w2, u0 w1 - u1 w0); "s + e t" is fl(s + fl(e t)) per axis), each output rounded to fp32 once.
 * Valid faces: a face with an index outside [0, V) or a vertex coordinate that is not finite is never a candidate (the
 * rule that gives it the empty box in pn_bvh_boxes).  The corners a, b, c are read from vertices and faces themselves, not
 * from the tracer's tris rows.
 * Point / triangle distance d2(p, f), with the closest point q and its barycentrics (u, v) in pn_trace_mesh's convention,
 * q = (1 - u - v) a + u b + v c - Ericson's region classification ("Real-Time Collision Detection", 5.1.5):
 *   ab = b - a, ac = c - a, n = ab x ac.  If n . n == 0 the face is its three edge segments, see below.  Otherwise, the
 *   first rule that holds decides:
 *   ap = p - a, d1 = ab . ap, d2 = ac . ap;            d1 <= 0 and d2 <= 0:              q = a, (u, v) = (0, 0)
 *   bp = p - b, d3 = ab . bp, d4 = ac . bp;            d3 >= 0 and d4 <= d3:             q = b, (1, 0)
 *   vc = d1 d4 - d3 d2;                                vc <= 0, d1 >= 0, d3 <= 0:        t = d1 / (d1 - d3), q = a + ab t, (t, 0)
 *   cp = p - c, d5 = ab . cp, d6 = ac . cp;            d6 >= 0 and d5 <= d6:             q = c, (0, 1)
 *   vb = d5 d2 - d1 d6;                                vb <= 0, d2 >= 0, d6 <= 0:        t = d2 / (d2 - d6), q = a + ac t, (0, t)
 *   va = d3 d6 - d5 d4, g = d4 - d3, h = d5 - d6;      va <= 0, g >= 0, h >= 0:          t = g / (g + h), q = b + (c - b) t, (1 - t, t)
 *   otherwise den = 1 / ((va + vb) + vc), u = vb den, v = vc den, q = (a + ab u) + ac v.
 *   d2 = r . r with r = p - q.
 *   Segment s .. e: se = e - s, L = se . se; t = 0 when L is not > 0 (a segment of length 0 is its end point s), else
 *   t = ((p - s) . se) / L clamped to [0, 1]; q = s + se t.  A face without area takes the nearest of ab, bc, ca in that
 *   order, a later segment replacing an earlier one only when its d2 is smaller (<): (u, v) = (t, 0), (1 - t, t), (0, 1 - t).
 * Answer for point p: the lexicographic minimum of (d2, f) over the candidates - equal fp64 d2 keeps the lowest face
 * index.  The search starts at best = max_distance^2 (the fp32 scalar squared in fp64; +inf: no limit), INCLUSIVE, with no
 * face held; a candidate replaces the held one when d2 < best, or d2 == best and no face is held or its index is lower.
 * Outputs: distance = fl(sqrt(d2)), face, closest = fl(q), bary = fl(u, v) of the winner.  No answer - a point with a
 * coordinate that is not finite, F = 0, no candidate within reach: face = -1, distance = +inf, closest = bary = 0.
 * pn_closest_point: brute force.  Every face in ascending index, staged through LDS in tiles of PN_MESHDIST_TILE; every
 *   valid face is taken as a candidate.
 * pn_closest_point_bvh: a walk of the nodes pn_bvh_tree wrote (layout above, unchanged), one point per thread, 64 threads
 *   per workgroup, the traversal stack [PN_BVH_MAX_DEPTH][64] in LDS as the tracer's; no scratch.
 *   Box bound: lb(p, box) = fl(((gx gx + gy gy) + gz gz) (1 - 2^-40)), g = max(max(lo - p, 0), p - hi) per axis, fp64 on
 *   the fp32 box; an empty box (lo.x > hi.x) is infinitely far and is never entered.
 *   Candidate rule: face f counts for p iff f is valid and lb(p, padded box of f) <= d2(p, f) (the box of pn_bvh_boxes).
 *   The walk starts at row 0.  A child is skipped only when its box is empty or lb > best (strict); a leaf that is not
 *   skipped is evaluated, must pass the candidate rule and then meets the replacement rule above; of two children to
 *   enter, the one with the smaller bound is entered first (the left one on a tie) and the other pushed.  The walk ends
 *   after F iterations at the latest (every internal node is entered at most once), also over a buffer that is no tree.
 *   The tree cannot matter: a node's box is the exact min / max union of its children's, down to the padded triangle
 *   boxes, and every operation of lb - fp64 subtraction from or of a fixed p, max, the square of a non-negative number,
 *   addition, the final factor - is monotone, so a parent's bound never exceeds a child's.  For the winner (d2*, f*):
 *   lb of every ancestor <= lb(f*) <= d2* <= best at all times, so every ancestor is entered whatever the topology and the
 *   order, and the replacement rule is a minimum over a set, which no order changes.
 *   The BVH result is the brute-force result wherever every valid face is a candidate.  The pad sees to that: q lies in the
 *   unpadded box up to the rounding of "s + e t" (a few 2^-53 of the coordinates), so the padded box is nearer to p than q
 *   is by at least about PN_BVH_PAD_ABS x mag = 4e-6 mag per axis it is outside on, and the factor 1 - 2^-40 covers lb's own
 *   three roundings; the margin is many orders above fp64 rounding.  tests/test_meshdist_cpu.py counts the violations on
 *   its scenes instead of trusting this (0), and reports the smallest margin.
 * Surface sampling, the choice of face in integers:
 *   pn_face_areas    area [F] fp64 = 0.5 sqrt(n . n), n = (b - a) x (c - a); 0 for a face that is not valid
 *   (the caller)     largest = the maximum of area (exact), 1 device double
 *   pn_face_weights  weight [F] int64 = floor(area / largest * 2^31) (the division first; 2^31 = PN_MESHDIST_WEIGHT_ONE), 0
 *                    where area is 0 or largest is not positive and finite: 0 <= weight <= 2^31
 *   (the caller)     cum_weight = the inclusive running sum of weight, int64 (exact), W = cum_weight[F - 1] <= F 2^31 < 2^62
 *   pn_sample_surface  sample i of count (systematic sampling): threshold t_i = floor(i W / count), computed as
 *                    i (W / count) + (i (W % count)) / count in int64 (i, count < 2^31: no product reaches 2^63); its face
 *                    is the first f with cum_weight[f] > t_i (binary search), so face f gets floor or ceil of
 *                    count weight[f] / W samples and a face of weight 0 none.  Barycentrics from the R2 sequence:
 *                    r_k = x_k - floor(x_k), x_k = 0.5 + A_k double(i), A_1 = PN_MESHDIST_R2_A1, A_2 = PN_MESHDIST_R2_A2 (1 / g
 *                    and 1 / g^2 of the plastic number g = 1.3247179572447460); when r_1 + r_2 > 1 both become 1 - r.
 *                    (u, v) = (r_1, r_2), point = (a + (b - a) u) + (c - a) v.  Outputs points [count, 3], face [count]
 *                    int32, bary [count, 2], rounded once.  A face that is not valid (cum_weight not of this mesh):
 *                    face = -1, zeros.
 * No atomics; the same bits on every call.  P = 0, count = 0 and F = 0 (areas, weights) launch nothing.
 * Errors: PN_ERR_BAD_SHAPE (a negative count, V, F or count >= 2^31, max_distance negative or NaN, F = 0 in
 * pn_closest_point_bvh and pn_sample_surface, W outside [1, 2^62]), PN_ERR_NULL. */
#define PN_MESHDIST_TILE 256
#define PN_MESHDIST_WEIGHT_ONE 2147483648.0
#define PN_MESHDIST_R2_A1 0.7548776662466927
#define PN_MESHDIST_R2_A2 0.5698402909980532
int pn_closest_point(int64_t P, const float* points, int64_t V, const float* vertices, int64_t F, const int32_t* faces,
                     float max_distance, float* distance, int32_t* face, float* closest, float* bary, void* stream);
int pn_closest_point_bvh(int64_t P, const float* points, int64_t V, const float* vertices, int64_t F, const int32_t* faces,
                         const float* nodes, float max_distance, float* distance, int32_t* face, float* closest,
                         float* bary, void* stream);
int pn_face_areas(int64_t F, int64_t V, const float* vertices, const int32_t* faces, double* area, void* stream);
int pn_face_weights(int64_t F, const double* area, const double* largest, int64_t* weight, void* stream);
int pn_sample_surface(int64_t count, int64_t W, int64_t F, int64_t V, const float* vertices, const int32_t* faces,
                      const int64_t* cum_weight, float* points, int32_t* face, float* bary, void* stream);

/* ---- winding number: the generalized winding number of a triangle mesh at arbitrary points (pn_winding.hip) -------------
 * w(p) = (1 / 4 pi) sum_f Omega(p, f), the signed solid angles of the faces as seen from p (Jacobson et al. 2013): 1 inside
 * and 0 outside a closed mesh wound so that (b - a) x (c - a) points outside, and a smooth blend of the two over holes,
 * soups and duplicated faces.  Meshes, points, valid faces and the arithmetic are the "mesh distance" section's: fp64 on
 * the fp32 inputs, separate operations in the written order, that section's dot and cross, each output rounded to fp32 once.
 * A face that is not valid contributes nothing anywhere.
 * Triangle term (van Oosterom and Strackee 1983), corners a, b, c of face f:
 *   A = a - p, B = b - p, C = c - p;  num = A . (B x C);  if num == 0: Omega = 0.  Otherwise
 *   la = sqrt(A . A), lb = sqrt(B . B), lc = sqrt(C . C),
 *   den = ((la lb) lc + (A . B) lc) + ((B . C) la + (C . A) lb),  Omega = 2 atan2(num, den).
 *   num == 0 is a point in the face's plane (on the face, an edge or a corner included): it takes the principal value 0, so
 *   a signed zero never decides between +2 pi and -2 pi, and w on a closed surface is the mean of its two sides.
 * w(p) = fl32(S / PN_WINDING_FOUR_PI), S the fp64 sum of the terms in the order stated below.  A point with a coordinate
 * that is not finite gets NaN; F = 0 gives 0.
 * pn_winding: the exact sum, brute force.  One point per thread, every face in ascending index staged through LDS in tiles
 *   of PN_WINDING_TILE as pn_closest_point does; S takes the valid faces' terms in that order.
 * pn_bvh_moments: one fp64 row per internal node of the nodes pn_bvh_tree wrote (layout unchanged), moments
 *   [max(F - 1, 1), 8] = (g[3], r2, N[3], A).  A leaf of face f hands up its vector area m = 0.5 ((b - a) x (c - a)) (0.5
 *   times each component), A_f = sqrt(m . m) and its centroid g_f = ((a + b) + c) / 3 per axis; zeros for a face that is not
 *   valid.  A node, from its left and right child in that order:
 *     N = N_left + N_right, A = A_left + A_right;
 *     box = the fp32 min / max union of the two child boxes of its nodes row; an empty box (lo.x > hi.x) gives a zero row;
 *     g = (A_left g_left + A_right g_right) / A per axis when A > 0, else (lo + hi) 0.5 of the box, in fp64;
 *     r2 = (ex ex + ey ey) + ez ez, e = max(g - lo, hi - g) per axis: the squared distance from g to the farthest corner
 *     of the box, so every vertex below the node lies within sqrt(r2) of g.
 *   Bottom-up in one launch, no host synchronisation and no floating-point atomics: one thread per internal node arrives
 *   at its own node for its leaf children, a thread that has written a row arrives at the parent (an atomicAdd on
 *   counters behind a fence, as pn_bvh_tree's refit), and the arrival that completes a node writes its row.  Every row is
 *   written once from the same operands in the same order, and every operation is an IEEE + - * / sqrt: two calls give
 *   the same bits, which are those of tests/_winding_ref.py.  F = 1 has no internal node: row 0 is zero.
 *   Work: counters [max(F - 1, 1)] int32 (zeroed by pn_bvh_moments itself).
 * pn_winding_bvh: a Barnes-Hut walk (in the manner of Barill et al. 2018, dipole term only), one point per thread, 64
 *   threads per workgroup, the traversal stack [PN_BVH_MAX_DEPTH][64] in LDS as pn_closest_point_bvh's; no scratch.
 *   Visiting a reference: a leaf adds Omega(p, f) if f is valid.  An internal node j takes x = g_j - p, d2 = x . x; if
 *   d2 > 0 and d2 >= beta2 r2_j (beta2 = the fp32 beta squared in fp64) it adds (N_j . x) / (d2 sqrt(d2)) and descends no
 *   further; otherwise it visits its left child next and pushes the right one.  The walk starts at row 0 (F = 1: at the
 *   single leaf), S takes the terms in visiting order - pre-order, left first, is part of the contract, the sum is not
 *   associative - and it ends after 2 F visits at the latest (a tree has 2 F - 1 references), also over a buffer that is
 *   no tree.  beta is finite and in [1, 1e6]: with beta >= 1 a point inside a node's box (d2 <= r2) does not take that
 *   node's far field, short of equality at the farthest corner.
 *   Unlike the tracer's and the distance walk's, this result DOES depend on the tree: it is an approximation, whose error
 *   falls as beta^-2.  It promises the same bits on every call and every build of the same mesh (tree and moments are
 *   deterministic), the exact sum's terms for beta so large that no node is far (1e6 on any mesh whose points lie within
 *   1e6 of its size), and the error table of tests/test_winding_cpu.py, recorded in DESIGN.md 6n.
 * Errors: PN_ERR_BAD_SHAPE (a negative count, V or F >= 2^31, F = 0 in pn_bvh_moments and pn_winding_bvh, beta outside
 * [1, 1e6] or NaN), PN_ERR_NULL.  P = 0 launches nothing. */
#define PN_WINDING_TILE 256
#define PN_WINDING_FOUR_PI 12.566370614359172
int pn_winding(int64_t P, const float* points, int64_t V, const float* vertices, int64_t F, const int32_t* faces,
               float* winding, void* stream);
int pn_bvh_moments(int64_t F, int64_t V, const float* vertices, const int32_t* faces, const float* nodes, double* moments,
                   int32_t* counters, void* stream);
int pn_winding_bvh(int64_t P, const float* points, int64_t V, const float* vertices, int64_t F, const int32_t* faces,
                   const float* nodes, const double* moments, float beta, float* winding, void* stream);

/* ---- radiance volume: the field baked into a voxel volume and ray-marched with no network (pn_volume.hip) -------------
 * data [nx, ny, nz, C] fp32 on pn_grid_points' vertex grid: vertex v = (i ny + j) nz + k at (x0 + i dx, ...), each axis
 * >= 2 vertices, fewer than 2^31 vertices, lo finite and steps positive and finite.  C = 1 + 3 K + E: channel 0 is sigma;
 * then K = (sh_degree + 1)^2 RGB triples (channel 1 + 3 k + c), real SH coefficients in the lighting section's order with
 * the constants below (sh_degree 0, 1 or 2); then E <= PN_VOLUME_MAX_ATTR attribute channels.  A vertex is one
 * contiguous run of C floats, so a trilinear tap reads 8 runs.
 * Occupancy: a cell is the cube between 8 neighbouring vertices, cells are grouped in bricks of PN_VOLUME_BRICK^3 cells
 * (partial bricks at the upper faces), nb_a = ceil((n_a - 1) / PN_VOLUME_BRICK) bricks per axis, brick
 * (bi nby + bj) nbz + bk.  pn_volume_occupancy writes ONE BYTE per brick: 1 iff a vertex of the brick (i in
 * [8 bi, min(8 bi + 8, nx - 1)], both ends included, likewise j, k) has sigma > 0, which is: iff a cell of the brick has a
 * corner with sigma > 0.  A NaN is not > 0.  pn_volume_bricks is the byte count (< 0: a bad grid).
 * Baking directions (volume.fibonacci_directions, fp64 on the host): for i = 0..D-1, y = 1 - (2 i + 1) / D,
 * r = sqrt(1 - y y), phi = i PN_VOLUME_GOLDEN_ANGLE, direction (r cos phi, y, r sin phi).  The bake's default D = 4 K, the
 * marcher's default step of half the smallest grid step, t_min = 1e-3 and the brick size are conventions, not measurements.
 *
 * pn_volume_march, rows r < R.  All arithmetic is fp64 on the fp32 inputs, separate operations in the written order
 * (-ffp-contract=off), each output rounded to fp32 once; one launch, no atomics: two calls give the same bits.
 * Lattice: len = sqrt((dx dx + dy dy) + dz dz) of the direction, dt = step / len, n = ceil((far - near) / dt) points,
 *   t_k = near + (k + 0.5) dt for 0 <= k < n, computed from k.  A row with a non-finite origin, direction, near or far,
 *   with len == 0, far <= near or n >= 2^31 writes 0 to every output and marches nothing.  The lattice does not depend on
 *   the volume or on the jumps.
 * Sample k: g_a = ((o_a + t_k d_a) - lo_a) / step_a per axis.  If g_a < 0 or g_a > n_a - 1 on any axis the sample adds
 *   nothing.  Otherwise c_a = min(floor(g_a), n_a - 2), f_a = g_a - c_a, corner weights w = (wx wy) wz with
 *   wx = 1 - f_x (low) or f_x (high), and trilinear(ch) = the sum of w v over the corners in the order i, j, k, low corner
 *   first, starting from 0.  sigma = trilinear(0); if !(sigma > 0) (a NaN included) the sample adds nothing.
 * Colour: Y_0..Y_{K-1} once per row at u = d / len (each component divided): PN_SH_C0, PN_SH_C1 {y, z, x},
 *   PN_SH_C2 (x y), PN_SH_C2 (y z), PN_SH_C3 (3 (z z) - 1), PN_SH_C2 (x z), PN_SH_C4 (x x - y y).  Per sample and channel
 *   s = sum_k Y_k trilinear(1 + 3 k + c) in k order from 0, colour = s > 0 ? s : 0.  Attributes are trilinear(1 + 3 K + e)
 *   as stored (a composited normal is not re-normalised).
 * Composite, ascending k from T = 1: alpha = 1 - exp(-sigma (dt len)), w = T alpha, rgb_c += w colour_c, attr_e += w a_e,
 *   acc += w, wt += w t_k, T = T (1 - alpha); then stop if T < t_min (t_min = 0 never stops).
 *   depth = min(max(q, near), far), q = wt / acc with a NaN quotient replaced by 0: k_composite_fwd's rule for fine_dep.
 *   There is no background term.
 * Jumps.  The coordinate g_a of sample k is a chain of correctly rounded operations on (k + 0.5) and so a monotone function
 *   of k.  (1) A sample beyond a box face on axis a: if the ray does not move towards the box on that axis (d_a of the wrong
 *   sign or 0) the march ends; otherwise k moves past kl, the largest proposal for which g_a(kl), evaluated by the sample
 *   formula, is still beyond the same face.  (2) With an occupancy table, a sample whose cell lies in an unoccupied brick:
 *   k moves past kl if the sample formula puts kl inside the box with its cell in the same brick.  Proposals come from the
 *   exit plane (an axis with d_a == 0 proposes nothing: no division), floor((t_plane - near) / dt - 0.5), then one less,
 *   then no jump.  By monotonicity every skipped sample is outside the box or in a cell of an unoccupied brick, whose
 *   corners are all <= 0 or NaN, and adds nothing: the outputs are the same bits with and without the table.
 * Outputs (null: not written): rgb [R, 3], depth [R], acc [R], attrs [R, E], and the diagnostic taps [R, 2] int32: the
 *   samples whose trilinear sigma was evaluated, and of those the ones with sigma > 0 (which read the colour too).  With a
 *   table the first count drops; the second does not change.
 * Errors: PN_ERR_BAD_SHAPE (a bad grid, sh_degree outside 0..2, E outside 0..PN_VOLUME_MAX_ATTR, step or a grid step not
 * positive and finite, t_min negative or not finite, R < 0), PN_ERR_NULL.  R = 0 launches nothing. */
#define PN_VOLUME_BRICK 8
#define PN_VOLUME_MAX_ATTR 8
#define PN_VOLUME_GOLDEN_ANGLE 2.399963229728653
#define PN_SH_C0 0.28209479177387814
#define PN_SH_C1 0.48860251190291992
#define PN_SH_C2 1.0925484305920792
#define PN_SH_C3 0.31539156525252005
#define PN_SH_C4 0.54627421529603959
int64_t pn_volume_bricks(int nx, int ny, int nz);
int pn_volume_occupancy(int nx, int ny, int nz, int channels, const float* data, uint8_t* occupancy, void* stream);
int pn_volume_march(int64_t R, int nx, int ny, int nz, int sh_degree, int E, const float* data, const uint8_t* occupancy,
                    float x0, float y0, float z0, float dx, float dy, float dz, const float* origins,
                    const float* directions, const float* near, const float* far, float step, float t_min, float* rgb,
                    float* depth, float* acc, float* attrs, int32_t* taps, void* stream);

/* ---- radiance volume: gradients: the reverse of the compositing sweep, for the dense store (pn_volume.hip) -----------
 * pn_volume_march_bwd takes pn_volume_march's arguments up to t_min (the optional occupancy table included), the upstream
 * gradients g_rgb [R, 3] and g_acc [R] (fp32; a null pointer counts as zeros) of a scalar L, and adds dL/d(data) for the
 * sigma and coefficient channels into sums [N, 1 + 3 K] (N = nx ny nz, vertex v, channel ch at v (1 + 3 K) + ch) as
 * 64-bit integers in units of `quantum`.  All arithmetic is fp64 on the fp32 inputs, separate operations in the written
 * order.  Per valid row (the forward's rule) the kernel runs pn_volume_march's own loop twice: the same lattice, gates,
 * jumps and early stop, term for term, from the same device function.  A sample "composites" if its sigma > 0; col_c is
 * its clamped colour, s_c the unclamped sum, w, alpha, T (before the sample) and wgt = T alpha the forward's values,
 * stepw = dt len.
 *   Pass 1.  u = ((g_r col_r + g_g col_g) + g_b col_b) + g_a per compositing sample; U = U + wgt u, ascending from 0.
 *   Pass 2.  Per compositing sample: P = P + wgt u (from 0), Tn = T (1 - alpha), ds = stepw (Tn u - (U - P)), which is
 *     dL/d(sigma of the sample): Tn u is what the sample adds itself, U - P what the samples behind it lose.  Its
 *     contributions, for corner q (weight w[q], vertex v):  sigma: x = w[q] ds into (v, 0);  coefficient (k, c):
 *     x = w[q] (Y_k (wgt g_c)) into (v, 1 + 3 k + c), only where s_c > 0 (the clamp's gate).
 * Attribute channels, depth, origins and directions get no gradient; a row the forward does not march adds nothing.
 * Accumulation.  quantum is a power of two in [2^-60, 1].  A contribution x becomes m = llrint(x / quantum) (round half
 *   to even) and, if m != 0, ONE relaxed agent-scope 64-bit integer fetch_add into sums (a vector atomic).  Integer
 *   addition is associative: sums depends neither on the order of the rows, nor on the schedule, nor on the table, and
 *   calls accumulate.  A contribution that is not finite or has |x / quantum| >= 2^52 adds nothing and ORs 1 into *flag
 *   (an integer atomic) instead.  Range: |sum| < 2^63 quantum, i.e. 2^23 at the customary quantum 2^-40; a sum beyond it
 *   wraps, silently: the caller's scale to avoid.  Each contribution is off by at most quantum / 2.
 * pn_volume_grad_finish: grad [N, C] fp32, grad[v, ch] = (float)((double)sums[v, ch] quantum) for ch < Cg (= 1 + 3 K),
 *   0 for Cg <= ch < C (the attribute channels), and NaN in EVERY entry if *flag != 0 (a poisoned backward, as torch
 *   has it; no host synchronisation is needed to look at the flag).  clear != 0 zeroes sums as it reads them and resets
 *   the flag with a one-thread launch behind the first.
 * Errors: as pn_volume_march, and PN_ERR_BAD_SHAPE for a quantum that is not a power of two in [2^-60, 1], Cg < 1,
 *   C < Cg or C > 36; PN_ERR_NULL for sums, flag or grad.  R = 0 launches nothing. */
int pn_volume_march_bwd(int64_t R, int nx, int ny, int nz, int sh_degree, int E, const float* data, const uint8_t* occupancy,
                        float x0, float y0, float z0, float dx, float dy, float dz, const float* origins,
                        const float* directions, const float* near, const float* far, float step, float t_min,
                        const float* g_rgb, const float* g_acc, double quantum, int64_t* sums, int32_t* flag, void* stream);
int pn_volume_grad_finish(int64_t N, int C, int Cg, int64_t* sums, double quantum, int32_t* flag, float* grad, int clear,
                          void* stream);

/* ---- sparse radiance volume: a brick table and a pool of the present bricks, fp32 or fp16 (pn_volume.hip) -------------
 * The same volume as above with the unoccupied bricks left out.  Bricks and their linear index are pn_volume_occupancy's:
 * nb_a = ceil((n_a - 1) / PN_VOLUME_BRICK), brick (bi nby + bj) nbz + bk.  A brick is PRESENT iff pn_volume_occupancy
 * says 1; its vertex range includes the shared far faces, so a positive vertex on a shared face makes every brick that
 * shares it present.
 * table int32 [nbx, nby, nbz]: the brick's slot in the pool, or -1.  Slots are 0 .. B - 1 in ascending brick index (an
 *   exclusive prefix sum of the occupancy), so the layout never depends on a schedule.
 * pool [B, 9, 9, 9, C], C fastest, fp32 or fp16 (`half` != 0): slot s, local vertex (li, lj, lk), 0 <= l <= 8, holds the
 *   global vertex (8 bi + li, 8 bj + lj, 8 bk + lk); local vertices past the grid's last vertex (partial bricks) hold 0.
 *   Value index (s 729 + (li 9 + lj) 9 + lk) C + ch, 64-bit; B 729 C < 2^40.
 * Consequences.  The 8 corners of cell c lie in ONE brick (c >> 3 per axis, local c & 7 and that + 1), so a trilinear tap
 *   is one table read and one base address.  Vertices on shared faces are stored once per present brick that holds them
 *   (729 / 512 = 1.42 x per brick); pn_volume_pack writes every copy from the same source value, so the copies agree.
 * fp16: each fp32 value is rounded to nearest even to binary16, subnormal results and fp32 subnormal inputs as IEEE 754
 *   says (numpy's astype(float16)); values of magnitude >= 65520 become infinities (volume.py refuses them).  Readers widen
 *   fp16 -> fp32 -> fp64 exactly.
 * pn_volume_pack writes the pool from `table` and ONE source: data [N, C] (the dense tensor), or rows [M, C] with
 *   vertex_row int32 [N] (the row of each vertex; an entry outside 0 .. M - 1, by convention -1, means every channel 0);
 *   the other source's pointers are null.  One workgroup per brick, absent ones leave at once; the lanes stride over the
 *   brick's 729 C values, so stores are contiguous; no atomics.  B = 0 launches nothing.
 * pn_volume_unpack writes data [N, C] fp32 from table and pool, one thread per vertex: the vertex is read from the present
 *   brick of LOWEST index that holds it (up to 8 candidates); a vertex in no present brick gets 0 in every channel.  A
 *   gather: no write race.  Both kernels treat a table entry outside 0 .. B - 1 as absent.
 * pn_volume_march_sparse is pn_volume_march, term for term, on the stored values: the same kernel template reads the
 *   corners through the table.  A sample whose cell lies in an absent brick: with skip != 0 the brick jump of (2) above,
 *   exactly as pn_volume_march takes it for an unoccupied brick; with skip == 0 it counts as one sigma tap of value 0
 *   (taps[.., 0] goes up, nothing is read, the next sample is k + 1).  The outputs are the bits pn_volume_march gives on
 *   the dense expansion (pn_volume_unpack's output): the corners of an absent brick are <= 0 or NaN in the source and 0
 *   in the expansion, so sigma > 0 fails either way.  With fp32 storage taps are those of pn_volume_march too (with the
 *   expansion's occupancy for skip != 0, without a table for skip == 0); with fp16 a brick whose positive sigmas all
 *   round to 0 stays present, and taps[.., 0] may exceed the expansion's.  The table is trusted as data is: every entry is
 *   -1 or a slot of the pool (volume.py checks it once, when the volume is made); pool may be null if none is present.
 * Errors: as pn_volume_march; pack / unpack: PN_ERR_BAD_SHAPE (a bad grid, channels < 1 or > 65536, B < 0, B above the
 *   brick count or B 729 C >= 2^40, M < 0, both sources given), PN_ERR_NULL (table, no source, the output, the pool when B > 0). */
int pn_volume_pack(int nx, int ny, int nz, int channels, const int32_t* table, int64_t B, const float* data,
                   const float* rows, int64_t M, const int32_t* vertex_row, int half, void* pool, void* stream);
int pn_volume_unpack(int nx, int ny, int nz, int channels, const int32_t* table, int64_t B, const void* pool, int half,
                     float* data, void* stream);
int pn_volume_march_sparse(int64_t R, int nx, int ny, int nz, int sh_degree, int E, const int32_t* table, const void* pool,
                           int half, int skip, float x0, float y0, float z0, float dx, float dy, float dz,
                           const float* origins, const float* directions, const float* near, const float* far, float step,
                           float t_min, float* rgb, float* depth, float* acc, float* attrs, int32_t* taps, void* stream);

/* ---- launch timing (bench.py roofline leg; off by default) ------------------------------------
 * pn_prof_enable(on): bit 0 switches the timing on or off; while on, every GEMM / chain launch is bracketed by HIP
 * events on its own stream (the other bits are ignored: the ablation switches of the tools/ micro-benchmarks exist only
 * in -DPN_ABLATE builds).  pn_prof_read waits for the recorded events and returns, for kernel class cls (0 k_gemm_nt,
 * 1 k_gemm_tn, 2 k_chain_fwd, 3 k_chain_dgrad, 4 k_chain_tangent, 5 k_chain_bwd, 6..10 k_chain_wgrad by tile configuration
 * 256x256 / 256x96 / 128x288 / 32x256 / 32x128 on fp32 tensors; 11 / 12 the 256x256 tile with Y / with X and Y in Q24), the summed duration in ms, the launch count and the summed algorithmic FLOPs (2*M*N*K, unpadded). */
/* diagnostic: `blocks` workgroups x 4 waves each issue 4*iters back-to-back fp32 MFMAs (no memory traffic) */
int pn_mfma_probe(float* out, int blocks, int iters, void* stream);
int pn_prof_enable(int on);
int pn_prof_read(int cls, double* total_ms, int64_t* launches, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* PANONERF_HIP_H */
