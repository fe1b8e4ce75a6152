/* libpsld_hip — C ABI of the MI355X (gfx950) PSLD hot path.
 *
 * Drop-in boundary.  The reference's only native FFI is the pybind module
 * `upfirdn2d_op.upfirdn2d(...)` (main/models/score_fn/song_sde/op/upfirdn2d.cpp:12-22) and
 * `fused.fused_bias_act(...)` (op/fused_bias_act.cpp:11-20); everything else on the path is
 * eager ATen called from Python.  This header is what a maintainer of the reference binds
 * instead (ctypes stub in INTEGRATION.md): every entry point takes raw device pointers, sizes
 * and a hipStream_t, never allocates, never synchronises, is re-entrant per stream, and
 * returns 0 on success (non-zero -> psld_last_error() has the message; the Python side raises
 * RuntimeError, or ValueError for PSLD_ERR_NUMERIC to mirror psld.py:166-171).
 *
 * Activations inside the network are NHWC ("channels-last": [B][H][W][C], C contiguous);
 * the public tensors (x, eps, samples) stay NCHW like the reference and are converted at the
 * network boundary by psld_nchw_to_nhwc_f32 / psld_nhwc_to_nchw_f32.
 */
#ifndef PSLD_HIP_H
#define PSLD_HIP_H

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
#else
typedef struct ihipStream_t* hipStream_t; /* opaque: pass the raw HIP stream handle */
#endif

#ifdef __cplusplus
extern "C" {
#endif


#define PSLD_ABI_VERSION 14 /* 2: limb-MFMA convolutions, math mode, bias-gradient / batched-copy entry points; 3: pointwise weight gradient and batched activation GEMM on limb kernels; 4: GroupNorm statistics from the limb kernels' epilogue; 5: per-sample-time reverse SDE, ScoreLoss nll / l1; 6: limb-plane activations; 7: device-resident dropout seed / Adam scalars (captured training step), GroupNorm-backward sums from the producing epilogue; 8: Winograd F(2x2,3x3) limb convolution; 9: launch tape; 10: GroupNorm apply (+SiLU) fused into the Winograd convolution's input staging; 11: GroupNorm backward kernel selector; 12: column sums of dx from the GroupNorm backward; 13: GroupNorm backward returns per-image sums (dgamma / dbeta / bias gradients and split-K slab reductions of a whole backward pass in batched launches), the GroupNorm-backward by-product of the limb epilogue and the launch tape (9) removed; 14: the optimiser kernels take the device error word (a refused step is a no-op + NaN loss), Winograd-domain 3x3 weight gradient (psld_conv3x3_wgrad_wino_*) */
#define PSLD_COEFF_STRIDE 12

int psld_version(void);
const char* psld_last_error(void);

/* Arithmetic of the MFMA tile kernels (GEMM / conv / wgrad).  Both take and return fp32 and accumulate in fp32.
 *   PSLD_MATH_F32    v_mfma_f32_32x32x2_f32 on the operands as they are (one fmaf per k);
 *   PSLD_MATH_BF16X6 every operand is split exactly into three bf16 limbs (hi + mid + lo == x, all 24 mantissa
 *                    bits) and each product is the six leading limb products on v_mfma_f32_32x32x16_bf16; the three
 *                    dropped terms are < 2^-23 of the product, i.e. below fp32 rounding of the product itself.
 *   PSLD_MATH_BF16X3 reduced-precision inference: bf16x6 for every launch, and the *_x3 entry points below (Winograd 3x3
 *                    forward, pointwise forward GEMM) keep the first TWO limbs of each operand (hi = rne_bf16(x), lo =
 *                    rne_bf16(x - hi): limbs 0 and 1 of the three-limb split, bit for bit) and the three products
 *                    hi*hi + (hi*lo + lo*hi); the dropped terms are each < 2^-16 of the product (rel-L2 ~1e-5 on a whole
 *                    network forward).  The library only stores this value: which launches use the two-limb entry
 *                    points is the caller's choice (psld_amd: forwards that record no backward pass).
 * Process-wide; the initial value comes from the environment variable PSLD_MATH ("f32" | "bf16x6" | "bf16x3" |
 * "bf16x3_train": mode PSLD_MATH_BF16X3 with record math PSLD_MATH_BF16X3, below | "f16": mode PSLD_MATH_BF16X3 with eval math
 * PSLD_EVAL_MATH_F16, below | "f16_train": "bf16x3_train" with record f16 on, below). */
#define PSLD_MATH_F32 0
#define PSLD_MATH_BF16X6 1
#define PSLD_MATH_BF16X3 2
int psld_set_math_mode(int mode);
int psld_get_math_mode(void);
/* Arithmetic of the passes that record a backward pass (training steps, the classifier's guidance pass): PSLD_MATH_BF16X6
 * (default: every launch of such a pass is the three-limb one, whatever the math mode) or PSLD_MATH_BF16X3 (opt-in: under a limb
 * math mode the pass takes the two-limb entry points where one exists - Winograd 3x3 forward and data gradient, pointwise forward
 * and data gradient, Winograd-domain weight gradient psld_conv3x3_wgrad_wino_x3_f32; gradients ~1e-5 rel-L2 from fp32).  Like the
 * math mode the library only stores the value; any other value is refused.  Initial value: PSLD_MATH_BF16X3 when PSLD_MATH is
 * "bf16x3_train", else PSLD_MATH_BF16X6. */
int psld_set_record_math(int mode);
int psld_get_record_math(void);
/* Eval math: arithmetic of the forwards that record NO backward pass (sampling).  PSLD_EVAL_MATH_LIMB (default): they follow the
 * math mode.  PSLD_EVAL_MATH_F16 (opt-in, meaningful under a limb math mode): they take the one-product fp16 entry points
 * (*_f16 below: Winograd 3x3 forward, eight-wave pointwise forward) where one exists and run as under PSLD_MATH_BF16X3 elsewhere.
 * Operands are rounded ONCE to fp16 (round to nearest even, clamped to +-65504: a finite operand never becomes an infinity),
 * products are exact in fp32, accumulation is fp32: 11 significant bits, the significand of TF32 - rel-L2 ~1e-3 on a whole
 * network forward, i.e. what the reference's default GPU arithmetic gives, NOT fp32-equivalent.  Values below 2^-24 in magnitude
 * round to zero (no per-tensor scaling).  The library only stores the value; any other value is refused.  Initial value:
 * PSLD_EVAL_MATH_F16 when PSLD_MATH is "f16" (which also selects math mode PSLD_MATH_BF16X3), else PSLD_EVAL_MATH_LIMB. */
#define PSLD_EVAL_MATH_LIMB 0
#define PSLD_EVAL_MATH_F16 1
int psld_set_eval_math(int kind);
int psld_get_eval_math(void);
/* Record f16: a fourth, independent setting (0 = off, the default; 1 = on; any other value is refused).  Meaningful under a limb
 * math mode with record math PSLD_MATH_BF16X3: a pass that records a backward pass then takes the one-product fp16 entry points
 * where one exists - Winograd 3x3 forward (psld_conv3x3_wino_f16_f32) and data gradient (psld_conv3x3_wino_f16s_f32 on fragments of
 * psld_pack_conv3x3_wino_dgrad_f16), eight-wave pointwise forward (psld_gemm_split_f16_f32) and data gradient
 * (psld_gemm_split_f16s_f32) - and the two-limb ones elsewhere; every weight gradient stays on limbs (the Winograd one is bound by
 * its producers, not by its MFMAs).  With record math PSLD_MATH_BF16X6 the flag has no effect.  Gradients of a mean-reduced loss
 * are ~2/N, below fp16's normal range: the *_f16s entries multiply their activation-side operand by 2^shift in fp32 before the one
 * rounding (clamped to +-65504) and fold 2^-shift into alpha - exact, so the rounding stays the only error; the caller chooses the
 * shift (psld_amd: ceil(log2 N) of the loss's divisor, at most 24).  11 significant bits, the arithmetic the reference trains in on
 * its own GPUs (TF32 convolutions): reference-GPU-equivalent, NOT fp32-equivalent, outside the 1e-4 parity contract, strictly
 * opt-in.  The library only stores the value.  Initial value: 1 when PSLD_MATH is "f16_train", else 0. */
int psld_set_record_f16(int on);
int psld_get_record_f16(void);

/* ---- fused epilogue of every MFMA tile kernel ------------------------------------------
 * value = ((alpha * acc + bias[n] + rowbias[m / rows_per_img][n] + residual[m][n]) * out_scale)
 *         (+ C[m][n] if accumulate)
 * Used for: conv bias (layers.py:103-109), the time-embedding add `h += Dense_0(act(temb))`
 * (layerspp.py:262-263), the residual `(x + h) / sqrt(2)` (layerspp.py:271-274, :88-91) and the
 * attention scale C^-1/2 (layerspp.py:82). */
typedef struct psld_epilogue {
    float alpha;
    const float* bias;
    const float* rowbias;
    int ld_rowbias;
    int rows_per_img;
    const float* residual;
    int ld_residual;
    long long residual_stride_batch;
    float out_scale;
    int accumulate;
    /* Optional (limb kernels psld_conv3x3_split_f32 / _limb_f32 / _wino_f32 / psld_gemm_split_f32 only; a call that splits
     * its K range over workgroups forms them in its reduction + epilogue pass instead: rows, N and gn_hw multiples of 64):
     * GroupNorm statistics of the OUTPUT as a by-product, for the GroupNorm that reads it next
     * (layerspp.py:258,264 GroupNorm_0/1; :77 of the attention block).  gn_part[((img*chunks + chunk)*(N/8) + f)*2 + {0,1}]
     * = sum / sum of squares of the 8 channels 8f..8f+7 over the chunk-th run of 64 rows of image img
     * (chunks = gn_hw / 64, gn_hw = rows per image, a multiple of 64; N a multiple of 128).  gn_fine = 4: sums of FOUR
     * channels 4f..4f+3 instead ((N/4) entries per run: tensors whose groups are 4 channels wide - 128 channels in 32
     * groups, CelebA-64's first level); 0 or 8: eight.
     * psld_gn_stats_from_partials_f32 turns them into the statistics of any group size that is a multiple of 8. */
    double* gn_part;
    int gn_hw;
    int gn_fine;
} psld_epilogue_t;

/* C[b] = epilogue(op(A[b]) * op(B[b])), fp32 MFMA (v_mfma_f32_32x32x2_f32), batched.
 * trans_a = 0: A is [M][K] (lda >= K); 1: A is [K][M].   trans_b = 0: B is [K][N]; 1: B is [N][K].
 * Replaces nn.Linear / NIN / 1x1 conv / attention einsums (layers.py:531-540, layerspp.py:82-87). */
int psld_gemm_f32(int trans_a, int trans_b, int M, int N, int K,
                  const float* A, int lda, long long stride_a,
                  const float* B, int ldb, long long stride_b,
                  float* C, int ldc, long long stride_c, int batch,
                  const psld_epilogue_t* epi, hipStream_t stream);

/* slabs[s] = A[ks:ke]^T B[ks:ke] for nsplit K-ranges (weight-gradient GEMMs with K = B*H*W). */
int psld_gemm_tn_splitk_f32(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                            float* slabs, int nsplit, hipStream_t stream);

/* NHWC implicit-GEMM convolution; input = concat(x1[c1], x2[c2]) along channels (x2 may be
 * NULL with c2 = 0: the up-path `torch.cat([h, hs.pop()], dim=1)` of ncsnpp.py:374 is never
 * materialised).  Weights are [cout][kh][kw][c1+c2].
 * transposed_stride = 1: y[n,oy,ox,:] = sum x[n, oy*stride+ky-pad, ox*stride+kx-pad, :] w[:,ky,kx,:]
 * transposed_stride = s>1 (data-gradient of a stride-s conv): input index (oy+ky-pad)/s when divisible.
 * Replaces nn.Conv2d 3x3/1x1 (layers.py:85-109) and F.conv2d(stride=2) of
 * up_or_down_sampling.py:177. */
int psld_conv2d_nhwc_f32(const float* x1, int c1, const float* x2, int c2,
                         int batch, int ih, int iw,
                         const float* w_ohwi, int cout, int kh, int kw,
                         int stride, int pad, int transposed_stride,
                         int oh, int ow, float* y, int ldy,
                         const psld_epilogue_t* epi, hipStream_t stream);

/* Same convolution with an optional scratch buffer (>= psld_conv2d_workspace_bytes): layers whose output
 * grid cannot fill the 256 CUs (small batches, 8x8 / 16x16 maps) split the K range over extra workgroups and
 * apply the epilogue while summing the partial slabs.  workspace == NULL behaves like psld_conv2d_nhwc_f32. */
long long psld_conv2d_workspace_bytes(int batch, int oh, int ow, int cout);
int psld_conv2d_nhwc_ws_f32(const float* x1, int c1, const float* x2, int c2,
                            int batch, int ih, int iw,
                            const float* w_ohwi, int cout, int kh, int kw,
                            int stride, int pad, int transposed_stride,
                            int oh, int ow, float* y, int ldy,
                            const psld_epilogue_t* epi, void* workspace, long long ws_bytes,
                            hipStream_t stream);

/* ---- 3x3 stride-1 pad-1 convolutions on bf16 limb MFMA (PSLD_MATH_BF16X6) --------------------------------
 * Direct convolution: a (rows+2) x (W+2) halo tile of the input is split into limbs once per 32-channel chunk and
 * read from LDS at the nine tap offsets; the weights come pre-split in MFMA fragment order
 * (psld_pack_conv3x3_frag, once per optimizer step; psld_conv3x3_frag_bytes bytes).  Same contract as
 * psld_conv2d_nhwc_ws_f32 for kh = kw = 3, stride = pad = 1 (input = concat(x1[c1], x2[c2]), fused epilogue,
 * optional split-K workspace of psld_conv2d_workspace_bytes).  Shapes: c1, c2 multiples of 32, cout a multiple
 * of 128, w in {8,16,32,64} with h*w dividing or divisible by 128 (psld_conv3x3_split_supported).
 * dgrad = 1 packs the weights of the data-gradient (taps flipped, channel roles swapped: "cout" of the call that
 * consumes them is the layer's cin).  Replaces nn.Conv2d 3x3 of every ResBlock (layerspp.py:29-39). */
long long psld_conv3x3_frag_bytes(int cout, int cin);
int psld_conv3x3_split_supported(int c1, int c2, int batch, int h, int w, int cout);
int psld_pack_conv3x3_frag(const float* w_oihw, void* wfrag, int cout, int cin, int dgrad, hipStream_t stream);
/* All weight tensors of a network in ONE launch (the per-tensor packs above are launch-bound: 228 x 7 us per step).
 * table_dev: device array of `entries` x 8 int64: {src pointer, dst pointer, n_out, k_in, taps | flip << 32,
 * stride_n, stride_k, first work item}; an entry has n_out*k_in/8 work items (one per lane slot, all taps and limbs)
 * and produces exactly what psld_pack_conv3x3_frag (taps 9) / psld_pack_gemm_frag (taps 1) would;
 * total_items = sum over entries.  k_in may carry (chunk0 << 20) | (chunks_total << 40) in its upper bits: the entry then
 * fills the 32-wide K chunks chunk0 .. chunk0 + k_in/32 of a fragment set whose K dimension has chunks_total chunks
 * (several parameters concatenated along K into one set - the q | k | v projections of an attention block read by ONE
 * data-gradient GEMM); both zero: the entry is the whole K dimension. */
int psld_pack_frag_batch(const long long* table_dev, int entries, long long total_items, hipStream_t stream);
int psld_conv3x3_split_f32(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w,
                           const void* wfrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                           void* workspace, long long ws_bytes, hipStream_t stream);

/* Winograd F(2x2, 3x3) form of psld_conv3x3_split_f32 (forward and, with dgrad fragments, data gradient): the same
 * convolution, contract and fused epilogue (no gnb_* by-product, no split-K workspace) with 2.25x fewer matrix
 * instructions.  Y = A^T[(G g G^T) (.) (B^T d B)]A per 2x2 output tile; the transformed operands are formed in fp32 and
 * carried as three exact bf16 limbs each, six limb products per product, fp32 accumulation: fp32-equivalent arithmetic
 * re-associated (what cuDNN may pick for the reference's nn.Conv2d 3x3, song_sde/layers.py:103-109), within ~2x of
 * the direct kernel's rounding error against fp64.  Weights come pre-transformed and pre-split in MFMA operand order
 * (psld_pack_conv3x3_wino, once per optimizer step; psld_conv3x3_wino_frag_bytes = 16/9 of the direct fragments).
 * Shapes: c1, c2 multiples of 32, cout a multiple of 128, h even, w in {8,16,32,64}, h*w dividing or divisible by 128.
 * 4x4 maps (h == w == 4) run as seven whole images per workgroup (252 of the 256 halo pixels of its raw image): every entry
 * point except the GroupNorm-fused ones, no gn_part.
 * Row strides: ldy and epi->ldres below 2^20 elements (every psld_conv3x3_wino_* launch: the epilogue addresses the up to
 * 416 pixels of a workgroup's region by 32-bit byte offsets from the first; larger strides are refused). */
long long psld_conv3x3_wino_frag_bytes(int cout, int cin);
int psld_conv3x3_wino_supported(int c1, int c2, int batch, int h, int w, int cout);
int psld_pack_conv3x3_wino(const float* w_oihw, void* ufrag, int cout, int cin, int dgrad, hipStream_t stream);
/* All Winograd fragment sets of a network in ONE launch.  table_dev: `entries` x 8 int64 {src pointer (OIHW weights),
 * dst pointer, n_out, k_in, flip, stride_n, stride_k, first work item}: forward fragments of a [cout][cin][3][3] weight
 * are {w, dst, cout, cin, 0, cin*9, 9, first}, data-gradient fragments {w, dst, cin, cout, 1, 9, cin*9, first}; an entry
 * has n_out*k_in/8 work items and produces exactly what psld_pack_conv3x3_wino would. */
int psld_pack_wino_batch(const long long* table_dev, int entries, long long total_items, hipStream_t stream);
int psld_conv3x3_wino_f32(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w,
                          const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                          hipStream_t stream);
/* The same with a workspace for small grids (one workgroup per CU: a launch below half a round - the 8x8 level at training
 * batches - leaves CUs idle): the channel chunks are split over psld_conv3x3_wino_ksplit workgroups per tile, plain partial
 * outputs go to the workspace (psld_conv3x3_wino_ws_bytes) and one reduction pass applies the epilogue, as
 * psld_conv3x3_split_f32 does for such shapes (epi->gn_part: formed by that pass).  Without a workspace or with ksplit == 1
 * it is psld_conv3x3_wino_f32. */
int psld_conv3x3_wino_ksplit(int c1, int c2, int batch, int h, int w, int cout);
long long psld_conv3x3_wino_ws_bytes(int c1, int c2, int batch, int h, int w, int cout);
int psld_conv3x3_wino_ws_f32(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w,
                             const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                             void* workspace, long long ws_bytes, hipStream_t stream);
/* The same convolution applied to act(GroupNorm(x)) without materialising it: x1 / x2 are the RAW tensors, scale* /
 * shift* the per-(image, channel) rows psld_gn_stats_nhwc_f32 / psld_gn_stats_from_partials_f32 produce ([batch][c1],
 * [batch][c2]; a two-source input is normalised per source, as the executor's concat-free up path does), act = 1: SiLU.
 * The activation a = act(x * scale + shift) is formed on the float4 a thread has just loaded for the kernel's raw halo
 * image; pixels outside the image stay zero (the reference pads the activated tensor).  For passes that need the
 * activated tensor nowhere else - the inference forward the samplers drive (GroupNorm_0/1 + act + Conv_0/1,
 * layerspp.py:245-263; no dropout in eval mode) - this removes psld_gn_apply_nhwc_f32's round trip through HBM.
 * Shapes: psld_conv3x3_wino_supported and h*w >= 128 (one image per workgroup region). */
int psld_conv3x3_wino_gn_supported(int c1, int c2, int batch, int h, int w, int cout);
int psld_conv3x3_wino_gn_f32(const float* x1, int c1, const float* scale1, const float* shift1, const float* x2, int c2,
                             const float* scale2, const float* shift2, int act, int batch, int h, int w,
                             const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                             hipStream_t stream);
/* ... with the workspace of psld_conv3x3_wino_ws_f32: small grids split their channel chunks the same way (bitwise the
 * unfused psld_gn_apply + psld_conv3x3_wino_ws_f32 pair). */
int psld_conv3x3_wino_gn_ws_f32(const float* x1, int c1, const float* scale1, const float* shift1, const float* x2,
                                int c2, const float* scale2, const float* shift2, int act, int batch, int h, int w,
                                const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                                void* workspace, long long ws_bytes, hipStream_t stream);

/* Two-limb (PSLD_MATH_BF16X3) forms of the Winograd forward: fragments of two limb planes [...][16 pos][2 limbs][64 lanes]
 * (cout*cin*16*4 bytes + the same prefetch pad; the planes are the hi and mid planes of psld_pack_conv3x3_wino: dgrad = 0
 * from psld_pack_conv3x3_wino_x3, dgrad = 1 - the data gradient is the same kernel on those fragments - from
 * psld_pack_conv3x3_wino_dgrad_x3; psld_pack_wino_batch_x3 takes psld_pack_wino_batch's table, rows of either orientation), V
 * split in two limbs, three products per accumulator.  Shapes: psld_conv3x3_wino_supported / psld_conv3x3_wino_gn_supported; workspace: NULL, or
 * psld_conv3x3_wino_ws_bytes bytes (the launches psld_conv3x3_wino_ksplit splits, split the same way).  Epilogue as above. */
long long psld_conv3x3_wino_frag_bytes_x3(int cout, int cin);
int psld_pack_conv3x3_wino_x3(const float* w_oihw, void* ufrag, int cout, int cin, hipStream_t stream);
int psld_pack_conv3x3_wino_dgrad_x3(const float* w_oihw, void* ufrag, int cout, int cin, hipStream_t stream);
int psld_pack_wino_batch_x3(const long long* table_dev, int entries, long long total_items, hipStream_t stream);
int psld_conv3x3_wino_x3_f32(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w,
                             const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                             void* workspace, long long ws_bytes, hipStream_t stream);
int psld_conv3x3_wino_gn_x3_f32(const float* x1, int c1, const float* scale1, const float* shift1, const float* x2,
                                int c2, const float* scale2, const float* shift2, int act, int batch, int h, int w,
                                const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                                void* workspace, long long ws_bytes, hipStream_t stream);
/* One-product fp16 (PSLD_EVAL_MATH_F16) forms of the Winograd forward: V = B^T d B and U = G g G^T are formed in fp32 as above and
 * stored as ONE plane of fp16 values (fragments [...][16 pos][1][64 lanes]: cout*cin*16*2 bytes + the same prefetch pad, from
 * psld_pack_conv3x3_wino_f16 - forward orientation only; psld_pack_wino_batch_f16 takes psld_pack_wino_batch's table), one
 * v_mfma_f32_16x16x32_f16 per accumulator, fp32 accumulation / output transform / epilogue as above.  Shapes, workspace and
 * K splits: those of the *_x3 entries. */
long long psld_conv3x3_wino_frag_bytes_f16(int cout, int cin);
int psld_pack_conv3x3_wino_f16(const float* w_oihw, void* ufrag, int cout, int cin, hipStream_t stream);
int psld_pack_wino_batch_f16(const long long* table_dev, int entries, long long total_items, hipStream_t stream);
int psld_conv3x3_wino_f16_f32(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w,
                              const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                              void* workspace, long long ws_bytes, hipStream_t stream);
int psld_conv3x3_wino_gn_f16_f32(const float* x1, int c1, const float* scale1, const float* shift1, const float* x2,
                                 int c2, const float* scale2, const float* shift2, int act, int batch, int h, int w,
                                 const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                                 void* workspace, long long ws_bytes, hipStream_t stream);
/* Record f16 (above): the data-gradient orientation of psld_pack_conv3x3_wino_f16 - the transposed, rotated weights as one fp16
 * plane, psld_conv3x3_wino_frag_bytes_f16(cin, cout) bytes (psld_pack_wino_batch_f16 takes rows of either orientation) - and
 * psld_conv3x3_wino_f16_f32 with an operand shift, 0 <= shift <= 24: V = B^T (x1 | x2) B times 2^shift, in fp32, is what is
 * rounded to fp16, and the epilogue's alpha is multiplied by 2^-shift (plain, channel-tail and split-chunk forms; in the last the
 * reduction pass applies it).  shift = 0 returns psld_conv3x3_wino_f16_f32's result bit for bit. */
int psld_pack_conv3x3_wino_dgrad_f16(const float* w_oihw, void* ufrag, int cout, int cin, hipStream_t stream);
int psld_conv3x3_wino_f16s_f32(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w,
                               const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi, int shift,
                               void* workspace, long long ws_bytes, hipStream_t stream);

/* "Limb planes": an NHWC activation [rows][c] (c a multiple of 32) stored already decomposed, as bf16
 * [rows][c/32 chunks][3 limbs hi|mid|lo][32 channels] (6 bytes per element; hi + mid + lo == x bit for bit).  The
 * producers of a 3x3 convolution's input write this form (psld_gn_apply_nhwc_f32 with y_limb) so that the convolution
 * stages its halo tile by LDS-DMA without splitting: psld_conv3x3_limb_f32 = psld_conv3x3_split_f32 with x1 / x2
 * given as limb planes (same weights fragments, same epilogue, bitwise the same result). */
long long psld_limb_bytes(long long rows, int c);
int psld_f32_to_limb(const float* x, long long rows, int c, void* y_limb, hipStream_t stream);
int psld_limb_to_f32(const void* y_limb, long long rows, int c, float* x, hipStream_t stream);
int psld_conv3x3_limb_f32(const void* x1_limb, int c1, const void* x2_limb, int c2, int batch, int h, int w,
                          const void* wfrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                          void* workspace, long long ws_bytes, hipStream_t stream);

/* Pointwise sibling of the kernel above: C = epilogue(A * B^T), A = concat(a1[m][k1], a2[m][k2]) row-major fp32,
 * B given as limb fragments of an [n][k] matrix (psld_pack_gemm_frag: element (n, k) is read at
 * b[n*stride_n + k*stride_k], so a [k][n] matrix such as NIN.W packs with stride_n = 1, stride_k = n;
 * psld_gemm_frag_bytes bytes).  Shapes: k1, k2 multiples of 32, k1 + k2 a multiple of 64, n a multiple of 128.
 * Replaces the 1x1 shortcut convolution (layerspp.py:268-270) and the NIN projections of the attention block
 * (layers.py:531-540, layerspp.py:78-88) and their data gradients. */
long long psld_gemm_frag_bytes(int n, int k);
int psld_gemm_split_supported(int k1, int k2, int m, int n);
int psld_pack_gemm_frag(const float* b, void* bfrag, int n, int k, long long stride_n, long long stride_k,
                        hipStream_t stream);
int psld_gemm_split_f32(const float* a1, int k1, const float* a2, int k2, int m, const void* bfrag, int n,
                        float* y, int ldy, const psld_epilogue_t* epi, void* workspace, long long ws_bytes,
                        hipStream_t stream);
/* Two-limb (PSLD_MATH_BF16X3) form of the forward GEMM (and, on fragments packed with n and k swapped, of its data gradient): fragments of the hi and mid planes only (n*k*4 bytes;
 * psld_pack_frag_batch_x3 takes psld_pack_frag_batch's table, taps = 1), rows split in two limbs, three products per
 * accumulator, every epilogue of psld_gemm_split_f32.  Always the eight-wave kernel of 128 x 256 tiles: shapes of
 * psld_gemm_split_supported with n a multiple of 256 (psld_gemm_split_f32 takes that kernel from 128 tiles on - below, its
 * four-wave kernel with split K fills the chip better); anything else stays on psld_gemm_split_f32. */
long long psld_gemm_frag_bytes_x3(int n, int k);
int psld_gemm_split_x3_supported(int k1, int k2, int m, int n);
int psld_pack_gemm_frag_x3(const float* b, void* bfrag, int n, int k, long long stride_n, long long stride_k,
                           hipStream_t stream);
int psld_pack_frag_batch_x3(const long long* table_dev, int entries, long long total_items, hipStream_t stream);
int psld_gemm_split_x3_f32(const float* a1, int k1, const float* a2, int k2, int m, const void* bfrag, int n,
                           float* y, int ldy, const psld_epilogue_t* epi, hipStream_t stream);
/* One-product fp16 (PSLD_EVAL_MATH_F16) form of the forward GEMM: fragments of one fp16 plane (n*k*2 bytes; psld_pack_frag_batch_f16
 * takes psld_pack_frag_batch's table, taps = 1), rows rounded once to fp16 (clamped to +-65504), one product per accumulator.
 * The eight-wave kernel and the shapes of the *_x3 entries. */
long long psld_gemm_frag_bytes_f16(int n, int k);
int psld_gemm_split_f16_supported(int k1, int k2, int m, int n);
int psld_pack_gemm_frag_f16(const float* b, void* bfrag, int n, int k, long long stride_n, long long stride_k,
                            hipStream_t stream);
int psld_pack_frag_batch_f16(const long long* table_dev, int entries, long long total_items, hipStream_t stream);
int psld_gemm_split_f16_f32(const float* a1, int k1, const float* a2, int k2, int m, const void* bfrag, int n,
                            float* y, int ldy, const psld_epilogue_t* epi, hipStream_t stream);
/* Record f16: the same launch with an operand shift, 0 <= shift <= 24 (the pointwise data gradient, on fragments packed with n and
 * k swapped through psld_pack_gemm_frag_f16's strides): the rows times 2^shift, in fp32, are what is rounded to fp16, alpha is
 * multiplied by 2^-shift.  Shapes: psld_gemm_split_f16_supported.  shift = 0 returns psld_gemm_split_f16_f32's result bit for bit. */
int psld_gemm_split_f16s_f32(const float* a1, int k1, const float* a2, int k2, int m, const void* bfrag, int n,
                             float* y, int ldy, const psld_epilogue_t* epi, int shift, hipStream_t stream);

/* Fused single-head spatial self-attention, forward: o[b][i][:] = sum_j softmax_j(scale * q[b][i] . k[b][j]) v[b][j][:] in
 * one kernel, the hw x hw score matrix never written (unless p != NULL: the probabilities [batch][hw][hw] fp32, what the
 * backward pass reads).  q / k / v: [batch*hw][c] fp32 with a common row stride ld (the fused q|k|v buffer: ld = 3c); o:
 * [batch*hw][c], row stride ldo.  Limb-MFMA arithmetic (three exact bf16 limbs, six products, fp32 accumulation), fp32 softmax.
 * hw in {256, 64} (16x16 / 8x8 maps), c in {256, 128, 480} (480: the attention width of an nf = 160 network; 64 queries per
 * workgroup at both map sizes, one workgroup per CU).  Reads exactly columns [0, c) of the hw rows of each image of q / k / v.  Replaces einsum -> softmax -> einsum of AttnBlockpp.forward
 * (song_sde/layerspp.py:82-86). */
int psld_attn_fwd_split_supported(int hw, int c);
int psld_attn_fwd_split_f32(const float* q, const float* k, const float* v, int ld, int batch, int hw, int c, float scale,
                            float* o, int ldo, float* p, hipStream_t stream);

/* Weight gradient of the same convolution, same slab contract as psld_conv2d_wgrad_nhwc_f32 (kh = kw = 3,
 * stride = pad = 1): slabs[s][cout][9][cin_total] restricted to columns [col0, col0 + cin), one slab per K range
 * of ceil(batch*h*w/32 / nsplit) 32-pixel tiles (every slab must be non-empty); the caller reduces
 * (psld_reduce_slabs_f32).  x2 / cin2 (null / 0 for none): second source of a channel concatenation, filling columns
 * [col0 + cin, col0 + cin + cin2).  Shapes: cout, cin, cin2 multiples of 64, w in {8,16,32,64}, h*w a multiple of 32. */
int psld_conv3x3_wgrad_split_supported(int cout, int cin, int batch, int h, int w);
/* Output channels per workgroup the kernel will use for this cout (64 or 128); a launch has
 * (cout / tile) * (cin / 64) * 3 * nsplit workgroups, 3 (tile 64) or 2 (tile 128) resident per CU: what the caller
 * needs to pick nsplit. */
int psld_conv3x3_wgrad_split_cout_tile(int cout);
int psld_conv3x3_wgrad_split_f32(const float* dy, int lddy, int cout, const float* x, int cin,
                                 const float* x2, int cin2, int batch, int h, int w, float* slabs,
                                 int cin_total, int col0, int nsplit, hipStream_t stream);
/* The same weight gradient with x (and x2) given as limb planes (psld_gn_apply_limb_nhwc / psld_f32_to_limb): the x
 * operand is staged without a split; dy stays fp32.  Bitwise the result of psld_conv3x3_wgrad_split_f32. */
int psld_conv3x3_wgrad_xlimb_f32(const float* dy, int lddy, int cout, const void* x_limb, int cin,
                                 const void* x2_limb, int cin2, int batch, int h, int w, float* slabs,
                                 int cin_total, int col0, int nsplit, hipStream_t stream);
/* Weight gradient of the same convolution in the Winograd F(2x2, 3x3) domain (wgrad_wino.hip; replaces the backward of
 * nn.Conv2d, reference main/models/score_fn/song_sde/layers.py:103-109): dU[xi] = sum over 2x2 output tiles of
 * (A dY A^T)[xi] (x) (B^T d B)[xi] for the 16 positions - 16 limb-MFMA products per 4 pixels instead of 36 - then
 * alpha * G^T dU G written (accumulate = 0) or added (1) to the OIHW gradient dw_oihw[cout][cin + cin2][3][3].  fp32 in, fp32
 * accumulate, exact three-limb operands like every limb kernel.  slabs: workspace of psld_conv3x3_wgrad_wino_ws_bytes;
 * nsplit: K splits of ceil(batch*h*w/128 / nsplit) 32-tile K tiles, none empty (psld_conv3x3_wgrad_wino_nsplit fills the chip
 * with one round of one-workgroup-per-CU tiles).
 * Shapes: cout % 128 == 0 (a workgroup owns 256 output channels of one position, 128 when cout is not a multiple of 256),
 * cin % 128 == 0, cin2 % 128 == 0 (second source of a channel concatenation; 0 / null for none),
 * h == w in {8,16,32,64}, batch*h*w % 128 == 0 (4x4 maps too: a K tile is eight images, batch % 8 == 0); dy rows of lddy floats. */
int psld_conv3x3_wgrad_wino_supported(int cout, int cin, int cin2, int batch, int h, int w);
int psld_conv3x3_wgrad_wino_nsplit(int cout, int cin_total, int batch, int h, int w);
long long psld_conv3x3_wgrad_wino_ws_bytes(int cout, int cin_total, int nsplit);
int psld_conv3x3_wgrad_wino_f32(const float* dy, int lddy, int cout, const float* x, int cin, const float* x2, int cin2,
                                int batch, int h, int w, float* slabs, int nsplit, float* dw_oihw, int accumulate,
                                float alpha, hipStream_t stream);
/* The same launch on two limbs per operand (record math PSLD_MATH_BF16X3): the transformed values keep limbs 0 and 1 of the
 * three-limb split, bit for bit, and a product is hi*mid + mid*hi + hi*hi (smallest first) - half the MFMAs.  Shapes, splits,
 * workspace (*_supported, *_nsplit, *_ws_bytes above) and the reduction are those of psld_conv3x3_wgrad_wino_f32. */
int psld_conv3x3_wgrad_wino_x3_f32(const float* dy, int lddy, int cout, const float* x, int cin, const float* x2, int cin2,
                                   int batch, int h, int w, float* slabs, int nsplit, float* dw_oihw, int accumulate,
                                   float alpha, hipStream_t stream);
/* Pointwise weight gradient on the limb kernels: slabs[s][i][j] (row stride ldc) = sum over the s-th range of
 * ceil(k/32 / nsplit) 32-row tiles of a[p][i] * b[p][j]  (a: [k][m] rows of lda floats, b: [k][n] rows of ldb floats;
 * b2 / ldb2 / n2 (null / 0 / 0 for none): further columns [n, n + n2) of B from a second tensor (concatenation);
 * m, n, n2 multiples of 128, k of 32; every slab non-empty).  Replaces the dW of the 1x1 convolutions and NIN
 * projections that autograd computes in the reference (layerspp.py:235,268-270 Conv_2; layers.py:531-540 NIN). */
int psld_gemm_tn_split_supported(int m, int n, int k);
int psld_gemm_tn_split_f32(int m, int n, int k, const float* a, int lda, const float* b, int ldb,
                           const float* b2, int ldb2, int n2, float* slabs, int ldc, int nsplit, hipStream_t stream);

/* Pointwise limb GEMMs for channel widths in steps of 32 ("tail" shapes: the 160 / 320 / 480-wide levels of an nf = 160
 * network), beside the entry points above, whose predicates and kernels are unchanged.
 *
 * Forward / data gradient: y[m][n] = epilogue(a[m][k] * B^T), one source.  psld_gemm_tail_supported: k % 32 == 0, n % 32 == 0,
 * k >= 128, n >= 128, m > 0 and NOT a shape of psld_gemm_split_supported(k, 0, m, n) (so n % 128 != 0 or k % 64 != 0).
 * Fragments: three limbs in psld_pack_gemm_frag's [n tile][half][chunk][block][limb][lane] layout with n rounded up to 128 and
 * k to 64: psld_gemm_frag_bytes_tail(n, k) = roundup(n, 128) * roundup(k, 64) * 6 bytes.  The packer writes the rows and the
 * K chunk beyond the tensor as zero limbs and reads b only inside [n][k].
 * psld_pack_frag_batch_tail: many tensors in one launch, psld_pack_frag_batch's table (8 x int64 per tensor: source, fragment
 * set, n, k, taps = 1, stride_n, stride_k, first work item) with the placement inside a shared set in the high bits of the n
 * and k fields: n | n0 << 20 | n_total << 40 (the tensor is rows n0 .. n0 + n of a set of n_total rows) and
 * k | chunk0 << 20 | chunks_total << 40 (it is the 32-wide K chunks chunk0 .. chunk0 + k/32 of chunks_total); zeros: the
 * tensor is the whole dimension.  The tensor that ends a dimension writes that dimension's zero padding, so the tensors of a
 * set write every byte of its psld_gemm_frag_bytes_tail(n_total, 32 * chunks_total).  A tensor has
 * psld_pack_frag_tail_items(n, n0, n_total, k, chunk0, chunks_total) work items.
 * psld_gemm_split_tail_f32: the four-wave kernel of psld_gemm_split_f32 on 128 x 128 tiles with the last column tile cut
 * short; every epilogue of psld_gemm_split_f32 (bias, row bias, residual, alpha, out_scale, accumulate, strided ldy) and
 * its split-K through the workspace for small m - except gn_part, which is refused (PSLD_ERR_ARG, nothing written).  Reads
 * exactly a[m][k] and columns [0, n) of residual / bias / row bias / y; on a launch without split-K every output element is
 * bit for bit column < n of psld_gemm_split_f32 on the same data zero-padded to roundup(n, 128) x roundup(k, 64).
 *
 * Weight gradient: psld_gemm_tn_split_f32's slabs (one B source) for m, n multiples of 32 from 128 up that are not both
 * multiples of 128, k % 32 == 0; loads beyond column m of a / n of b are masked, slab rows / columns beyond them not stored. */
int psld_gemm_tail_supported(int k, int m, int n);
long long psld_gemm_frag_bytes_tail(int n, int k);
int psld_pack_gemm_frag_tail(const float* b, void* bfrag, int n, int k, long long stride_n, long long stride_k,
                             hipStream_t stream);
long long psld_pack_frag_tail_items(int n, int n0, int n_total, int k, int chunk0, int chunks_total);
int psld_pack_frag_batch_tail(const long long* table_dev, int entries, long long total_items, hipStream_t stream);
int psld_gemm_split_tail_f32(const float* a, int k, int m, const void* bfrag, int n, float* y, int ldy,
                             const psld_epilogue_t* epi, void* workspace, long long ws_bytes, hipStream_t stream);
int psld_gemm_tn_split_tail_supported(int m, int n, int k);
int psld_gemm_tn_split_tail_f32(int m, int n, int k, const float* a, int lda, const float* b, int ldb, float* slabs,
                                int ldc, int nsplit, hipStream_t stream);

/* Batched GEMM on the limb kernels with BOTH operands fp32 activations (split inside the kernel):
 * c[b][i][j] = alpha * sum_p A(i,p) B(p,j);  ta: a is stored [k][m] (else [m][k]); tb: b is stored [n][k] (else [k][n]);
 * same operand conventions as psld_gemm_f32, not both transposed.  m, n multiples of 128, k of 32.  Replaces the
 * einsum contractions of the attention block, layerspp.py:82-86 (QK^T, softmax(QK^T) V) and their gradients. */
int psld_bgemm_split_supported(int ta, int tb, int m, int n, int k);
int psld_bgemm_split_f32(int ta, int tb, int m, int n, int k, const float* a, int lda, long long stride_a,
                         const float* b, int ldb, long long stride_b, float* c, int ldc, long long stride_c,
                         int batch, float alpha, hipStream_t stream);
/* The same product with the last column tile cut short (the N = 480 products of attention at 480 channels: P V and the
 * gradients dV, dQ, dK on 16x16 maps).  psld_bgemm_split_tail_supported: not both transposed, m % 128 == 0, n % 32 == 0,
 * n >= 128, k % 32 == 0 and NOT a shape of psld_bgemm_split_supported (so n % 128 != 0).  Same arguments as
 * psld_bgemm_split_f32.  Columns (tb: rows) of b at or beyond n are not read and columns of c at or beyond n not written;
 * every element written is bit for bit that of psld_bgemm_split_f32 on b zero-padded to roundup(n, 128) columns. */
int psld_bgemm_split_tail_supported(int ta, int tb, int m, int n, int k);
int psld_bgemm_split_tail_f32(int ta, int tb, int m, int n, int k, const float* a, int lda, long long stride_a,
                              const float* b, int ldb, long long stride_b, float* c, int ldc, long long stride_c,
                              int batch, float alpha, hipStream_t stream);

/* Weight gradient of the convolution above for one input source:
 * slabs[s][co][tap][col0 + ci] = sum over the s-th range of output pixels of dy[pix][co] * x[pix+tap][ci]. */
int psld_conv2d_wgrad_nhwc_f32(const float* dy, int lddy, int cout,
                               const float* x, int cin, int batch, int ih, int iw,
                               int kh, int kw, int stride, int pad, int oh, int ow,
                               float* slabs, int cin_total, int col0, int nsplit,
                               hipStream_t stream);

/* ---- launch plans of the fp32 tile engine ------------------------------------------------------------------------
 * Which kernel form psld_gemm_f32 / psld_gemm_tn_splitk_f32 / psld_conv2d_nhwc_ws_f32 / psld_conv2d_wgrad_nhwc_f32 take for
 * a call: the launches select their kernel through the same host code these queries run, so a test (or a caller sizing a
 * workspace) can see the form a shape reaches.  Each query takes the launch's own arguments without the stream.  Host
 * arithmetic only: device pointers (those inside *epi included) are looked at for 16-byte alignment and null-ness and are
 * never dereferenced; nothing is launched and no HIP call is made.  Returns a form code, or -1 for arguments the launch
 * refuses (psld_last_error has the message).
 * Form code = kernel kind | operand flags:
 *   PSLD_TILE_GENERIC       128 x 128 tile, one LDS buffer, any shape / alignment (every TT GEMM, K % 32 != 0, channel counts
 *                           that are no multiple of 32, transposed stride, more than 31 taps, non-power-of-two weight-gradient maps)
 *   PSLD_TILE_FAST128       128 x 128 tile of the branch-free kernel (all operands float4-addressable)
 *   PSLD_TILE_FAST256       128 x 256 tile of it (K-contiguous B: NT GEMM and convolution; N % 256 == 0 and >= 512 such tiles)
 *   PSLD_TILE_FAST64        64 x 128 tile of it (NT GEMM / convolution of more than 64 rows whose 128-row grid has <= 256 tiles)
 *   PSLD_TILE_FAST64_SPLITK convolution only: the 64 x 128 kernel over 2..8 K ranges into the workspace, then the reduction +
 *                           epilogue pass (psld_conv2d_plan also returns the range count and the K values per range)
 *   PSLD_TILE_A_VEC / PSLD_TILE_B_VEC: the A / B operand (GEMM: A / B; convolution: input / weights; weight gradients: dy / x) is
 *                           loaded as float4 (set on every fast form; on the generic form one flag per operand). */
enum psld_tile_form {
    PSLD_TILE_GENERIC = 0,
    PSLD_TILE_FAST128 = 1,
    PSLD_TILE_FAST256 = 2,
    PSLD_TILE_FAST64 = 3,
    PSLD_TILE_FAST64_SPLITK = 4,
    PSLD_TILE_KIND_MASK = 15,
    PSLD_TILE_A_VEC = 16,
    PSLD_TILE_B_VEC = 32
};
int psld_gemm_plan(int trans_a, int trans_b, int M, int N, int K,
                   const float* A, int lda, long long stride_a,
                   const float* B, int ldb, long long stride_b,
                   const float* C, int ldc, long long stride_c, int batch,
                   const psld_epilogue_t* epi);
int psld_gemm_tn_splitk_plan(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                             const float* slabs, int nsplit);
/* *nsplit / *kper (either may be NULL): K ranges of the launch (1: not split) and K values per range. */
int psld_conv2d_plan(const float* x1, int c1, const float* x2, int c2,
                     int batch, int ih, int iw,
                     const float* w_ohwi, int cout, int kh, int kw,
                     int stride, int pad, int transposed_stride,
                     int oh, int ow, const float* y, int ldy,
                     const psld_epilogue_t* epi, const void* workspace, long long ws_bytes,
                     int* nsplit, int* kper);
int psld_conv2d_wgrad_plan(const float* dy, int lddy, int cout,
                           const float* x, int cin, int batch, int ih, int iw,
                           int kh, int kw, int stride, int pad, int oh, int ow,
                           const float* slabs, int cin_total, int col0, int nsplit);

/* out[perm(i)] = alpha * sum_s slabs[s][i]; layout: 0 = keep [co][tap][ci], 1 = write OIHW [co][ci][tap]. */
int psld_reduce_slabs_f32(const float* slabs, int nsplit, long long n, float* out,
                          int layout, int cout, int taps, int cin, float alpha, hipStream_t stream);

/* ---- weight layout (state_dict keeps the reference's OIHW / [in,out] shapes) ------------ */
/* OIHW -> [co][tap][ci] (forward operand). */
int psld_pack_oihw_to_ohwi_f32(const float* w, float* out, int cout, int cin, int taps, hipStream_t stream);
/* OIHW -> [ci][flip(tap)][co] (data-gradient operand: the conv of dy with the flipped, transposed filter). */
int psld_pack_oihw_to_dgrad_f32(const float* w, float* out, int cout, int cin, int taps, hipStream_t stream);

/* ---- layout at the network boundary -------------------------------------------------------*/
int psld_nchw_to_nhwc_f32(const float* x, float* y, int batch, int c, int hw, hipStream_t stream);
int psld_nhwc_to_nchw_f32(const float* x, float* y, int batch, int c, int hw, hipStream_t stream);

/* ---- GroupNorm (+SiLU), NHWC (nn.GroupNorm(min(C//4,32), eps=1e-6) + nn.SiLU:
 *      layerspp.py:67,219,231,243,264; ncsnpp.py:276-280,427) ------------------------------- */
/* workspace: psld_gn_workspace_bytes(batch, hw, c, groups). Outputs per-(n,g) mean/rstd and the
 * per-(n,c) affine scale = rstd*gamma, shift = beta - mean*rstd*gamma. */
long long psld_gn_workspace_bytes(int batch, int hw, int c, int groups);
int psld_gn_stats_nhwc_f32(const float* x, int batch, int hw, int c, int groups, float eps,
                           const float* gamma, const float* beta,
                           float* mean, float* rstd, float* scale, float* shift,
                           void* workspace, hipStream_t stream);
/* Second half of psld_gn_stats_nhwc_f32 on partial sums a limb kernel's epilogue produced (psld_epilogue_t.gn_part,
 * fine_width = its gn_fine: 8 or 4 channels per sum; channels per group must be a multiple of it). */
int psld_gn_stats_from_partials_f32(const double* gn_part, int fine_width, int batch, int hw, int c, int groups, float eps,
                                    const float* gamma, const float* beta, float* mean, float* rstd,
                                    float* scale, float* shift, hipStream_t stream);
/* y = dropout(act(x*scale[n,c] + shift[n,c])); act: 0 = identity, 1 = SiLU.  Dropout
 * (nn.Dropout, layerspp.py:265): element i of the NHWC tensor is kept iff
 * psld_dropout_keep(seed, i, p) (counter-based hash, reproducible in the backward pass, no mask
 * tensor) and scaled by 1/(1-p); drop_p = 0 disables it. */
/* seed_dev (may be NULL): one device word added to `seed` by the kernel - the per-step part of the dropout seed lives
 * in device memory so that a hipGraph-captured training step draws a fresh mask on every replay. */
int psld_gn_apply_nhwc_f32(const float* x, const float* scale, const float* shift, float* y,
                           int batch, int hw, int c, int act, float drop_p, unsigned long long seed,
                           const unsigned long long* seed_dev, hipStream_t stream);
/* The same pass writing bf16 limb planes (see psld_conv3x3_limb_f32) instead of fp32: y_limb holds
 * psld_limb_bytes(batch*hw, c) bytes; c a multiple of 32.  The dropout mask is the one psld_gn_apply_nhwc_f32 and
 * psld_gn_bwd_nhwc_f32 derive from (seed, element index). */
int psld_gn_apply_limb_nhwc(const float* x, const float* scale, const float* shift, void* y_limb, int batch,
                            int hw, int c, int act, float drop_p, unsigned long long seed,
                            const unsigned long long* seed_dev, hipStream_t stream);
/* Which kernel psld_gn_bwd_nhwc_f32 takes when the backward runs in one pass over (dy, x):
 *   PSLD_GN_BWD_AUTO      the resident-workgroup kernel (gn_bwd_pipe_kernel: the next slab's x lands in LDS by global_load_lds
 *                         while the workgroup reduces and stores) where its shape rules hold and there is no third operand, else
 *   PSLD_GN_BWD_ONE_SLAB  the register-resident one-slab kernel (gn_bwd_fused_kernel) for every shape.
 * Both give bitwise equal dx / sums / colsum_img (tests/test_kernels_gpu.py compares them through this switch).  Process-wide;
 * the initial value comes from the environment variable PSLD_GN_BWD_PIPE ("0" = one slab). */
#define PSLD_GN_BWD_AUTO 0
#define PSLD_GN_BWD_ONE_SLAB 1
int psld_set_gn_bwd_kernel(int kind);
int psld_get_gn_bwd_kernel(void);

/* Backward of y = dropout(act(GN(x))) (autograd of nn.GroupNorm + nn.SiLU + nn.Dropout, layerspp.py:256-265):
 *   dx = d/dx (+ add_scale * add when add != NULL: the gradient of an identity branch parallel to the normalisation,
 *        e.g. the residual `(x + h) / sqrt(2)` of layerspp.py:271-274) (+ the previous dx when accumulate_dx);
 *   sums [batch][2][c] (written): per image and channel sum_p dz and sum_p dz * xhat, dz = dy * mask/keep * act'(.).  The
 *        parameter gradients are their sums over the batch - dbeta[c] = sum_n sums[n][0][c], dgamma[c] = sum_n sums[n][1][c] -
 *        formed by psld_param_reduce2_f32 for one layer or, for all layers of a backward pass in ONE launch, by
 *        psld_param_reduce_batch_f32 (the reference computes them inside one autograd graph; here they leave the
 *        dependency chain of the backward pass);
 *   colsum_img (may be NULL; only where psld_gn_bwd_colsum_supported): [batch] rows of ld_img floats, columns [0, c)
 *        written: the column sums over the pixels of image n of the dx values THIS call stores (add / previous dx included) -
 *        the bias gradient and per-image time-embedding gradient of the layer whose output gradient this dx is
 *        (layerspp.py:258-263: Conv_0 + Dense_0(act(temb))[:, :, None, None]; :268-274: Conv_1 / Conv_2 when this call is
 *        the last writer of the residual stream's gradient) without a pass over dx.  Without a third operand from a
 *        closed form, per channel sum_p dx = k0 sum_p dz - hw k1 - k2 sum_p xhat, of sums the kernel reduces anyway; with
 *        one by summing the stored values (fp32 per thread, fp64 across threads, fixed order). */
int psld_gn_bwd_nhwc_f32(const float* dy, const float* x, const float* mean, const float* rstd,
                         const float* gamma, const float* beta, int batch, int hw, int c, int groups,
                         int act, float drop_p, unsigned long long seed, const unsigned long long* seed_dev,
                         float* dx, int accumulate_dx, const float* add, float add_scale, float* sums,
                         float* colsum_img, int ld_img, void* workspace, hipStream_t stream);
int psld_gn_bwd_colsum_supported(int batch, int hw, int c, int groups);
/* The same backward on WHOLE NHWC ROWS (round 5): a workgroup owns 64 pixels x 128 channels, the K = hw / 64 workgroups of an
 * (image, 128-channel block) exchange their per-group partial sums through `sync` and write dx from their registers - the
 * reads are 512-byte runs of consecutive rows instead of one 128-byte segment per row (5.9-6.4 against 4.3-4.6 TB/s).  Maps
 * above 32x32 take 128 pixels per workgroup (K = hw / 128): there the alternative is the three-pass form.
 *   psld_gn_bwd_team_rows: K (> 1) when the form takes the shape - c a multiple of 128, groups of 4 | cpg | 128 channels,
 *        128 <= hw <= 1024 a multiple of 64 or 1024 < hw <= 4096 a multiple of 128 - and the kernel selector is
 *        PSLD_GN_BWD_AUTO; else 0.
 *   sums [batch * K][2][c]: sum_p dz and sum_p dz * xhat per (image, team member, channel): dbeta / dgamma are the sums over
 *        ALL batch * K rows (psld_param_reduce*_f32 with rows = batch * K).
 *   colsum_rows (may be NULL): [batch * K] rows of ld_rows floats: column sums of the stored dx over the member's pixels
 *        (a bias gradient is alpha * the sum over all rows; per-IMAGE sums - the time-embedding gradient - need the one-slab
 *        kernels, psld_gn_bwd_nhwc_f32).
 *   sync: psld_gn_bwd_team_sync_bytes() of device memory, zeroed ONCE by the caller and then left to the kernels (slots,
 *        tag counter, error word 0: non-zero after a member gave up waiting - several seconds - for its team); one stream at a
 *        time may use a given buffer.  The launch is one RESIDENT grid; results are deterministic (fixed summation order) but
 *        not bitwise those of the one-slab kernels (group terms from fp32-rounded member sums). */
int psld_gn_bwd_team_rows(int batch, int hw, int c, int groups);
long long psld_gn_bwd_team_sync_bytes(void);
int psld_gn_bwd_team_f32(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                         const float* beta, int batch, int hw, int c, int groups, int act, float drop_p, unsigned long long seed,
                         const unsigned long long* seed_dev, float* dx, int accumulate_dx, const float* add, float add_scale,
                         float* sums, float* colsum_rows, int ld_rows, void* sync, hipStream_t stream);

/* ---- parameter gradients that are sums over the batch (or over split-K slabs), off the backward chain ----------------
 * dst1[col] (and dst2[col] when non-NULL) = alpha * sum over r in [0, rows) of src[r * ld + col], col in [0, c): fp64
 * accumulation in a fixed order (16 row lanes r, r + 16, ... combined in lane order): bitwise repeatable.  What
 * nn.GroupNorm's dgamma / dbeta, the bias gradients and nn.Linear's bias gradient are in the reference's autograd graph.
 * psld_param_reduce2_f32: two jobs of the same shape in one launch (dbeta = rows of `sums`, dgamma = rows of `sums + c`).
 * psld_param_reduce_batch_f32: `jobs` rows of a DEVICE table of 8 int64
 *   [src pointer, rows, ld, c, dst1 pointer, dst2 pointer or 0, bit pattern of (float) alpha, first 64-column block],
 * blocks = sum over the jobs of ceil(c / 64). */
int psld_param_reduce2_f32(const float* src_a, const float* src_b, int rows, int ld, int c, float* dst_a, float* dst_b,
                           float alpha, hipStream_t stream);
int psld_param_reduce_batch_f32(const long long* table_dev, int jobs, int blocks, hipStream_t stream);
/* Split-K slab reductions of MANY weight gradients in one launch (psld_reduce_slabs_f32 per job, bitwise the same sums): rows of
 * a DEVICE table of 10 int64 [slabs pointer, nsplit, n, out pointer, layout, taps, cin, bit pattern of (float) alpha, first
 * unit, units]; a job has psld_reduce_slabs_batch_units(n, layout, taps, cin) units (0: the job does not qualify - n and cin
 * must be multiples of 4, taps <= 9; slabs 16-byte aligned); units = their sum.  With layout 1 the OIHW scatter goes through
 * LDS and leaves as contiguous 16-byte stores.  layout 2: a column block of wider slabs - element (r, j) of the
 * [n / cols][cols] result is the sum over slabs of slabs[s][r * ld + j] with cols passed as `taps`, ld as `cin`, a slab
 * (n / cols) * ld floats long and the slabs pointer at the block's first column (the q | k | v weight gradients of
 * AttnBlockpp from ONE [c][3c] GEMM, layerspp.py:78-80). */
int psld_reduce_slabs_batch_units(long long n, int layout, int taps, int cin);
int psld_reduce_slabs_batch_f32(const long long* table_dev, int jobs, long long units, hipStream_t stream);


/* ---- FIR resampling: the replacement of the pybind op upfirdn2d_op.upfirdn2d
 *      (op/upfirdn2d.cpp:12-22, op/upfirdn2d_kernel.cu:209-369).  Same semantics: zero-insert
 *      upsample by `up`, pad (negative = crop), convolve with `kernel` (i.e. correlate with the
 *      flipped kernel), decimate by `down`.  layout 0: NCHW ([N*C][H][W], the reference op's view),
 *      1: NHWC.  out_h = (in_h*up + pad0 + pad1 - kh)/down + 1.  Backward = same entry with the
 *      flipped kernel, up<->down swapped and the g_pad of op/upfirdn2d.py:111-116. */
int psld_upfirdn2d_f32(const float* x, float* y, int batch, int c, int in_h, int in_w,
                       const float* kernel_host, int kh, int kw,
                       int up_x, int up_y, int down_x, int down_y,
                       int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                       int layout, int accumulate, hipStream_t stream);
/* The (compiled-but-unused) second native op of the reference, for inventory parity:
 * y = act(x + b[(i / step_b) % size_b]) * scale, act 1 = linear, 3 = leaky-relu(alpha)
 * (op/fused_bias_act_kernel.cu:18-49, forward only). */
int psld_fused_bias_act_f32(const float* x, const float* b, float* y, long long n, int size_b, int step_b,
                            int act, float alpha, float scale, hipStream_t stream);
/* The op with all seven arguments of the reference's binding (op/fused_bias_act.cpp:11-20: input, bias, refer, act,
 * grad, alpha, scale): grad = 1 is the first derivative - x is the incoming gradient, `refer` the forward output, as
 * FusedLeakyReLUFunctionBackward calls it (op/fused_act.py:27-33) - grad = 2 the second (zero for both activations). */
int psld_fused_bias_act_grad_f32(const float* x, const float* b, const float* refer, float* y, long long n, int size_b,
                                 int step_b, int act, int grad, float alpha, float scale, hipStream_t stream);

/* ---- pointwise / reductions ---------------------------------------------------------------*/
/* y = (a*sa + b*sb) (b may be NULL); accumulate: y += ... */
int psld_axpby_f32(const float* a, float sa, const float* b, float sb, float* y, long long n,
                   int accumulate, hipStream_t stream);
int psld_silu_f32(const float* x, float* y, long long n, hipStream_t stream);
int psld_silu_bwd_f32(const float* x, const float* dy, float* dx, long long n, hipStream_t stream);
/* out[b][c] = alpha * sum over the hw rows of image b of x[(b*hw+p)*ld + c] (bias / temb-bias gradients). */
long long psld_colsum_workspace_bytes(int batch, int hw, int c);
int psld_colsum_f32(const float* x, int ld, int batch, int hw, int c, float* out, float alpha,
                    void* workspace /* >= psld_colsum_workspace_bytes, NULL = slow scalar path */,
                    hipStream_t stream);
/* Bias gradient in three launches (two chained psld_colsum_f32 calls take four): out[c] = alpha * sum over (batch, hw) of x[b][p][0..c) (row stride ld), and, when
 * per_image is not NULL, per_image[b*ld_per_image + c] = the unscaled per-image sums (ld_per_image = 0 means c; the
 * time-embedding gradient needs them, layerspp.py:262-263).  Same workspace as psld_colsum_f32; c % 4 == 0, c <= 1024, 16-byte aligned x. */
int psld_bias_grad_f32(const float* x, int ld, int batch, int hw, int c, float* per_image, int ld_per_image,
                       float* out, float alpha, void* workspace, hipStream_t stream);
/* The same over a [batch*hw][3*seg] buffer (row stride ld) whose three column segments are the output gradients of three
 * layers computed by one GEMM (the q | k | v projections of AttnBlockpp, layerspp.py:78-80): out0 / out1 / out2 [seg]. */
int psld_bias_grad_seg_f32(const float* x, int ld, int batch, int hw, int seg, float* out0, float* out1, float* out2,
                           float alpha, void* workspace, hipStream_t stream);
/* Many contiguous copies in one launch: table_dev = `entries` x 4 int64 {src pointer, dst pointer, float4 count, first
 * float4 index}; total4 = sum of the counts.  Used to gather the Dense_0 (time-embedding projection,
 * layerspp.py:225-228) weights of all ResBlocks into one [sum C_out][4*nf] matrix per optimizer step, so that their
 * 57 forward Linear calls and 57 data gradients become one GEMM each. */
int psld_copy_batch_f32(const long long* table_dev, int entries, long long total4, hipStream_t stream);

/* dst[r][0:cols] (+)= src[r][0:cols] with row strides: channel concat (ncsnpp.py:374) and its split. */
int psld_copy2d_f32(const float* src, int ld_src, float* dst, int ld_dst, long long rows, int cols,
                    int accumulate, hipStream_t stream);
/* 3x3 im2col of a few-channel NHWC tensor (9*c <= ld_out): cols[m][ch*9 + tap] (zero-filled to ld_out columns), so
 * that the 6-channel stem / first-pyramid convolutions (ncsnpp.py:317, layerspp.py:149-163) and the data / weight
 * gradients of the 6-channel head (ncsnpp.py:430) run as K = 64 GEMMs on the tile engine.  flip = 1 (stride 1 only)
 * stores tap 8 - t in the column of tap t (what a data gradient reads).  The column order ch*9 + tap is OIHW's. */
int psld_im2col3x3_small_f32(const float* x, int batch, int ih, int iw, int c, int oh, int ow, int stride, int pad,
                             int flip, float* out, int ld_out, hipStream_t stream);
/* 3x3 im2col / col2im of an NHWC tensor with c % 4 == 0 channels, K order (tap, channel) = the OHWI weight order of
 * psld_pack_oihw_to_ohwi_f32: cols[m][tap*c + ch] = x[n, oy*stride + ky - pad, ox*stride + kx - pad, ch] (zero outside);
 * col2im is its adjoint (written, fixed summation order).  They turn the stride-2 convolution of the input pyramid
 * (`Downsample` with fir: up_or_down_sampling.py:177 `F.conv2d(x, w, stride=2)`, layerspp.py:149-163) and its data
 * gradient into psld_gemm_split_f32 calls. */
int psld_im2col3x3_f32(const float* x, int batch, int ih, int iw, int c, int oh, int ow, int stride, int pad,
                       float* cols, hipStream_t stream);
int psld_col2im3x3_f32(const float* dcols, int batch, int ih, int iw, int c, int oh, int ow, int stride, int pad,
                       float* dx, hipStream_t stream);
/* y[n,oy,ox,o] = bias[o] + sum_{tap,c} x[n,oy+ky-1,ox+kx-1,c] * w_ohwi[o][tap][c]: 3x3 stride-1 pad-1 convolution with
 * 3 or 6 output channels (the network head `conv3x3(in_ch, channels)`, ncsnpp.py:430), exact fp32 fmaf chains + a
 * fixed cross-lane sum; cin % 4 == 0, cin <= 256, weights in the OHWI order of psld_pack_oihw_to_ohwi_f32. */
int psld_conv3x3_fewout_supported(int cin, int cout);
int psld_conv3x3_fewout_f32(const float* x, const float* w_ohwi, const float* bias, float* y, int batch,
                            int h, int w, int cin, int cout, hipStream_t stream);
/* dst[r][j] = alpha * src[r][j], j < cols, arbitrary cols / leading dimensions (pads and un-pads the small K = 54
 * weight matrices of the calls above). */
int psld_scale_copy2d_f32(const float* src, int ld_src, float* dst, int ld_dst, long long rows, int cols, float alpha,
                          hipStream_t stream);

/* rows of length L: y = softmax(x) ; dx = y * (dy - sum(y*dy)) (layerspp.py:84). */
int psld_softmax_rows_f32(const float* x, float* y, long long rows, int L, hipStream_t stream);
int psld_softmax_rows_bwd_f32(const float* y, const float* dy, float* dx, long long rows, int L, hipStream_t stream);

/* ---- time embedding (layerspp.py:39-41, layers.py:500-514) ----------------------------------*/
/* out[b] = cat[sin(p), cos(p)], p = ((logf(t[b]) * W[e]) * 2) * pi   (use_log = 1, Fourier)
 *                               p = t[b] * W[e]                      (use_log = 0, positional) */
int psld_time_embed_f32(const float* t, const float* W, float* out, int batch, int e, int use_log,
                        hipStream_t stream);

/* ---- PSLD SDE (main/models/sde/psld.py) -----------------------------------------------------*/
typedef struct psld_sde_params {
    double beta_0, beta_1, nu, gamma, m_inv, numerical_eps;
    int decomp_lower;      /* 1 = 'lower' (Cholesky), 0 = 'upper' */
} psld_sde_params_t;

/* Per-sample f64 scalars of the perturbation kernel, PSLD_COEFF_STRIDE doubles per sample:
 * [0] = b_t (psld.py:42-44), [1] = exp(-(nu+gamma)/4 * b_t) (psld.py:65-67), [4..7] = c11,c12,c21,c22
 * of get_coeff (psld.py:154-186), [8..10] = (xx_t, xm_t, mm_t) of _cov (psld.py:86-152).  nan_flag (device int, caller-zeroed) is set to 1 if any
 * coefficient is NaN (psld.py:166-171 raises ValueError). */
int psld_perturb_coeffs_f64(const double* t, int batch, const psld_sde_params_t* p,
                            double xx_0, double mm_0, double* coeffs, int* nan_flag, hipStream_t stream);
/* u_t = mu_t + L_t eps (psld.py:262-287), NCHW.  x0,m0 [B,C,H,W] f32 (m0 NULL = zeros: HSM),
 * eps [B,2C,H,W] f32; writes z_t f32 (losses.py:114) and optionally u_t / mu_t f64. */
int psld_perturb_f32(const float* x0, const float* m0, const float* eps, const double* coeffs,
                     const psld_sde_params_t* p, int batch, int c, int hw,
                     float* z_f32, double* u_f64, double* mu_f64, hipStream_t stream);
/* loss = mean|sum (eps - eps_pred)^2 over n elements (losses.py:118-129); partials workspace
 * >= psld_reduce_workspace_bytes(n); also writes d(loss)/d(eps_pred) * upstream if grad != NULL. */
long long psld_reduce_workspace_bytes(long long n);
int psld_sqerr_loss_f32(const float* eps, const float* eps_pred, long long n, int reduce_mean,
                        float* loss, float* grad, float grad_scale, void* workspace, hipStream_t stream);

/* One Euler-Maruyama predictor update of the reverse SDE (samplers/sde.py:16-26 +
 * psld.py:230-260,330-364), NCHW, float64 state:
 *   f = drift(x, beta), g = diffusion;  score = -L^{-T} eps_pred (f32, coefficients cast to f32);
 *   f_bar = -f + g^2 * score (x0.5 if probability_flow); x_mean = x + f_bar*dt;
 *   x = x_mean + g*sqrt(dt)*z   (z NULL -> drift-only "denoise" step, sde.py:28-36)
 * Also writes x as f32 for the next network call (psld.py:354). */
typedef struct psld_em_coeffs {
    double beta;                 /* beta(T - t) */
    double m_inv, gamma, nu, m;  /* SDE constants */
    float c11, c12, c21, c22;    /* get_inv_coeff(...) cast to f32 (psld.py:253-258) */
    double dt;
    int score_mode;              /* 0 = score_xm (6-ch eps), 1 = score_m lower (3-ch eps -> momentum only),
                                    2 = score_x upper */
    int probability_flow;
} psld_em_coeffs_t;
int psld_em_step_f64(double* x, const float* eps_pred, const double* z, const psld_em_coeffs_t* k,
                     int batch, int c, int hw, float* x_f32_out, hipStream_t stream);
/* reverse_sde outputs themselves (f_bar, g_bar) for callers that want them (psld.py:345-364). */
int psld_reverse_sde_f64(const double* x, const float* eps_pred, const psld_em_coeffs_t* k,
                         int batch, int c, int hw, double* f_bar, double* g_bar, hipStream_t stream);
/* The same outputs with PER-SAMPLE times, as PSLD.sde / reverse_sde take them (psld.py:330-364, t[B]): t_rev[b] is the
 * already reversed time T - t of sample b (device f64); beta_t, _cov and get_inv_coeff are evaluated per sample on the
 * device (no host read of t).  eps_pred NULL: the forward SDE's own (f, g) of psld.py:330-343 (t_rev = t).  nan_flag
 * as in psld_perturb_coeffs_f64 (psld.py:214-219 raises ValueError).  batch <= 65535. */
int psld_reverse_sde_rows_f64(const double* x, const float* eps_pred, const double* t_rev,
                              const psld_sde_params_t* p, double xx_0, double mm_0, int score_mode,
                              int probability_flow, int batch, int c, int hw, double* f_bar, double* g_bar,
                              int* nan_flag, hipStream_t stream);
/* Symmetric-splitting (SSCS) sampler, SURVEY.md 8(f) rank 1 (samplers/sde.py:227-370):
 * analytic half step u <- M u + L z (M = exp-scaled 2x2 mean matrix of :236-263, L = factor of the
 * transition covariance :265-291 through get_coeff) and the Euler score step of :313-329. */
typedef struct psld_sscs_coeffs {
    double a_xx, a_xm, a_mx, a_mm;
    double c11, c12, c21, c22;
} psld_sscs_coeffs_t;
int psld_sscs_analytic_f64(double* x, const double* z, const psld_sscs_coeffs_t* k,
                           int batch, int c, int hw, float* x_f32_out, hipStream_t stream);
int psld_sscs_score_step_f64(double* x, const float* eps_pred, const psld_em_coeffs_t* k,
                             int batch, int c, int hw, hipStream_t stream);
/* Few-step exponential-integrator sampler (ei_ode; not in the reference): one multistep update
 *   u <- Phi u + sum_{j < n_hist} C_j eps_j
 * of the float64 state in place.  eps is a HOST array of n_hist (1..3) device pointers to float32 network outputs, newest
 * first, each promoted to double; Phi and C_j are host-computed float64 coefficients (never cast to float32).
 *   augmented = 1: state and eps are [B, 2c, hw] = [x | m]; phi and c[j] are row-major 2x2 matrices acting on the pair
 *                  (x, m) of one pixel: x' = phi[0] x + phi[1] m + sum_j (c[j][0] ex_j + c[j][1] em_j), m' likewise
 *                  with entries [2], [3];
 *   augmented = 0: (VP-SDE) state and eps are [B, c, hw]; only phi[0] and c[j][0] are used.
 * Optionally writes the float32 rounding of the new state for the next network call.  16-byte accesses when every
 * pointer is 16-byte aligned (and, augmented, c * hw % 4 == 0), element-wise otherwise. */
typedef struct psld_ei_coeffs {
    double phi[4];
    double c[3][4];
    int n_hist;
    int augmented;
} psld_ei_coeffs_t;
int psld_ei_step_f64(double* x, const float* const* eps, const psld_ei_coeffs_t* k,
                     int batch, int c, int hw, float* x_f32_out, hipStream_t stream);
/* The stochastic member of the family (ei_sde; order 1 only): one update
 *   u <- Phi u + C eps + S z
 * of the float64 state in place, with ONE float32 eps buffer (promoted to double) and float64 standard-normal noise z in
 * the state's layout.  phi, c, s as psld_ei_coeffs_t's phi and c[0]; s is lower-triangular (s[1] is not read):
 * x' = ... + s[0] zx, m' = ... + s[2] zx + s[3] zm; augmented = 0 uses entry [0] of each.  z == NULL drops the noise
 * term: the result is then psld_ei_step_f64's at n_hist = 1 on the same phi and c, bit for bit.  Same optional float32
 * copy, same 16-byte / element-wise forms (z counts among the pointers). */
typedef struct psld_ei_sde_coeffs {
    double phi[4];
    double c[4];
    double s[4];
    int augmented;
} psld_ei_sde_coeffs_t;
int psld_ei_sde_step_f64(double* x, const float* eps, const double* z, const psld_ei_sde_coeffs_t* k,
                         int batch, int c, int hw, float* x_f32_out, hipStream_t stream);
/* Measurement-guided (posterior) sampling for y = A x0 + noise (not in the reference; csrc/restore.hip):
 * the two kernels around the one network evaluation with its input gradient that a guided call costs.  float32 tensors,
 * float64 arithmetic in registers, one host-computed float64 coefficient set per call (one time for the whole batch):
 *   q_u, q_e: the Tweedie estimate x0^ = q_u[0] u_x + q_u[1] u_m - q_e[0] e_x - q_e[1] e_m of the clean image,
 *   l = (l11, l21, l22): the lower Cholesky factor of the perturbation covariance, kappa = scale / (sigma_y^2 + r_t^2);
 *   augmented = 1: state, eps, cotangent, dx and out are [B, 2c, h, w] = [x | m];
 *   augmented = 0: (VP-SDE) they are [B, c, h, w] and entry [0] of q_u, q_e, l (= sigma_t) is used.
 * psld_restore_measure_f32 writes g = A^T (y - A x0^) ([B, c, h, w]) and the cotangent (q_e[0] g | q_e[1] g) in one pass:
 *   op = PSLD_RESTORE_MASK: A x = mask . x, y and mask [B, c, h, w] (mask of {0, 1}; NULL for the other operators);
 *   op = PSLD_RESTORE_GRAY: A x = (x_R + x_G + x_B) / sqrt(3), c == 3, y [B, 1, h, w];
 *   op = PSLD_RESTORE_POOL: A x = (1 / k) sum over each k x k block, k = 2 or 4 dividing h and w, y [B, c, h/k, w/k]
 *   (k is read by the pool operator only); every A has orthonormal rows.
 * psld_restore_combine_f32 writes out_x = e_x - kappa (q_e[0] g - l11 dx_x - l21 dx_m), out_m = e_m - kappa (q_e[1] g -
 * l22 dx_m) (augmented = 0: out = e - kappa (q_e[0] g - l[0] dx)), dx the vector-Jacobian product of the cotangent.
 * 16-byte accesses when every pointer is 16-byte aligned and the shape allows (mask, combine: c * h * w % 4 == 0 augmented,
 * any length flat; gray: h * w % 4 == 0; pool: w % 4 == 0), element-wise otherwise: any h, w and any alignment works. */
#define PSLD_RESTORE_MASK 0
#define PSLD_RESTORE_GRAY 1
#define PSLD_RESTORE_POOL 2
typedef struct psld_restore_coeffs {
    double q_u[2];
    double q_e[2];
    double l[3];
    double kappa;
    int augmented;
} psld_restore_coeffs_t;
int psld_restore_measure_f32(const float* u, const float* eps, const float* y, const float* mask, int op, int k,
                             const psld_restore_coeffs_t* q, int batch, int c, int h, int w, float* g, float* cot,
                             hipStream_t stream);
int psld_restore_combine_f32(const float* eps, const float* g, const float* dx, const psld_restore_coeffs_t* q,
                             int batch, int c, int hw, float* out, hipStream_t stream);
/* The deconv operator ("Deconvolution"; csrc/deconv.hip): A x = k (*) x per channel, PERIODIC boundary, one PSF k for
 * every image and channel.  A A^T is no multiple of the identity, so these are entry points of their own and not a fourth
 * operator code of psld_restore_measure_f32 (which keeps refusing code 3).  h and w: each a power of two from 4 to 128
 * (psld_restore_deconv_supported returns 1 for such a pair and 0 otherwise; anything else is refused before the launch).
 *   hhat: float64 [h][w/2 + 1][2], the Hermitian half of FFT2(k wrapped onto the h x w torus, centred at its middle tap),
 *         computed once on the host; yhat: float64 [planes][h][w/2 + 1][2], the same half of FFT2(y) per plane, written by
 *         psld_restore_deconv_spectrum_f32 once per measurement.  Both 16-byte aligned.
 * psld_restore_deconv_f32 is the measure step: with x0^ as above and x^ = FFT2(x0^) it writes
 *         g = IFFT2( conj(hhat) (sigma_y2 + r2) / (sigma_y2 + r2 |hhat|^2) (yhat - hhat x^) )      [batch, c, h, w]
 *   and the cotangent (q_e[0] g | q_e[1] g) of the state's shape; a frequency whose denominator is exactly 0 contributes 0.
 *   sigma_y2 = sigma_y^2 and r2 = r_t^2 (kappa of q = scale / (sigma_y2 + r2) is read by psld_restore_combine_f32 alone,
 *   which serves this operator unchanged); both >= 0 with a positive finite sum.  For |hhat| = 1 this is A^T (y - A x0^).
 * psld_restore_deconv_apply_f32 writes A x (adjoint = 0) or A^T x (adjoint = 1) of float32 planes x [planes][h][w].
 * float32 planes in memory, float64 in registers and LDS; one workgroup per plane at a time (any number of planes), the
 * plane's packed transform in LDS: (h (w/2 + 1) + max(h, w) / 2) * 16 bytes, 131 KiB at 128 x 128; no scratch beyond LDS.
 * 16-byte accesses to the float32 tensors when their pointers are 16-byte aligned, 4-byte ones otherwise: same values. */
int psld_restore_deconv_supported(int h, int w);
int psld_restore_deconv_spectrum_f32(const float* y, int planes, int h, int w, double* yhat, hipStream_t stream);
int psld_restore_deconv_f32(const float* u, const float* eps, const double* yhat, const double* hhat,
                            const psld_restore_coeffs_t* q, double sigma_y2, double r2, int batch, int c, int h, int w,
                            float* g, float* cot, hipStream_t stream);
int psld_restore_deconv_apply_f32(const float* x, const double* hhat, int adjoint, int planes, int h, int w, float* out,
                                  hipStream_t stream);
/* Super-resolution ("Super-resolution"; csrc/deconv.hip): A x = D_s (k (*) x), the periodic blur of the deconv
 * operator followed by keeping the samples (s i, s j), s = 2 or 4; the measurement is [batch, c, h/s, w/s].  A A^T is circulant
 * on the low-resolution grid with eigenvalues lam, so (sigma_y2 I + r2 A A^T)^-1 is a pointwise division there.  h and w: each
 * a power of two up to 128 with h/s >= 4 and w/s >= 4 (psld_restore_sr_supported returns 1 for such a triple, 0 otherwise;
 * anything else is refused before the launch).
 *   hhat: as for deconv, float64 [h][w/2 + 1][2], 16-byte aligned;
 *   lam:  float64 [h/s][w/(2s) + 1], lam[m1][m2] = (1 / s^2) sum_{a, b < s} |h^[m1 + a h/s][m2 + b w/s]|^2, real and symmetric,
 *         computed once on the host.
 * psld_restore_sr_f32 is the measure step: z = IFFT2(hhat FFT2(x0^)), rho[i][j] = y[i][j] - z[s i][s j],
 *         v = IFFT2'( (sigma_y2 + r2) / (sigma_y2 + r2 lam) FFT2'(rho) ) on the low-resolution grid (denominator 0: 0),
 *         g = IFFT2( conj(hhat) FFT2(D_s^T v) )                                                   [batch, c, h, w]
 *   and the cotangent (q_e[0] g | q_e[1] g), all three transform pairs of a plane in the LDS of one workgroup, the
 *   low-resolution plane in the storage of the full one (the deconv kernels' LDS budget, nothing added).
 * psld_restore_sr_apply_f32: adjoint = 0: out [planes][h/s][w/s] = A x of x [planes][h][w]; adjoint = 1: out [planes][h][w] =
 *   A^T x of x [planes][h/s][w/s].  h and w are the FULL plane's sides in both directions.
 * float32 tensors, float64 in registers and LDS; 16-byte accesses when the float32 pointers are 16-byte aligned, 4-byte ones
 * otherwise: same values. */
int psld_restore_sr_supported(int h, int w, int s);
int psld_restore_sr_f32(const float* u, const float* eps, const float* y, const double* hhat, const double* lam,
                        const psld_restore_coeffs_t* q, double sigma_y2, double r2, int batch, int c, int h, int w, int s,
                        float* g, float* cot, hipStream_t stream);
int psld_restore_sr_apply_f32(const float* x, const double* hhat, int adjoint, int planes, int h, int w, int s, float* out,
                              hipStream_t stream);
/* Edges of the path.  Writer: position half of the f64 [B,c_total,H,W] state ->
 * uint8 [B,H,W,c] = trunc(clip((x*0.5+0.5)*255, 0, 255)) (callbacks.py:103-107, util.py:147-158).
 * Loader: uint8 [B,H,W,c] -> f32 [B,c,H,W] = img/127.5-1 (norm) or img/255, optional per-image
 * horizontal flip (util.py:25-30, datasets/cifar10.py:33-46). */
int psld_samples_to_uint8(const double* x, unsigned char* out, int batch, int c, int c_total, int hw,
                          int denorm, hipStream_t stream);
int psld_uint8_to_images_f32(const unsigned char* img, float* out, const unsigned char* flip,
                             int batch, int c, int h, int w, int norm, hipStream_t stream);
/* Adaptive Runge-Kutta building blocks for the black-box probability-flow ODE sampler (SURVEY 8(f)
 * rank 2, samplers/ode.py:40-76; the reference round-trips every RHS evaluation through host numpy via
 * torchdiffeq's scipy bridge).  v / coef are HOST arrays of nv <= 8 device pointers / doubles.
 *   out = base + sum_j coef[j]*v[j]            (base may be NULL; optional f32 copy)
 *   out[0] = sum_i ((sum_j coef[j]*v[j][i]) / (atol + rtol*max(|p_i|,|q_i|)))^2   (device scalar) */
int psld_lincomb_f64(double* out, const double* base, const double* const* v, const double* coef, int nv,
                     long long n, float* out_f32, hipStream_t stream);
int psld_scaled_norm_sq_f64(const double* const* v, const double* coef, int nv, const double* p,
                            const double* q, double atol, double rtol, long long n, double* out,
                            void* workspace /* >= psld_reduce_workspace_bytes(n) */, hipStream_t stream);
/* Probability-flow likelihood: the device kernels around ONE vector-Jacobian product of the network per
 * evaluation of the augmented ODE's right-hand side.  One time per call, its scalars from the host as in the samplers:
 * ``k`` is the psld_em_coeffs_t of the (forward) time t (dt and probability_flow are ignored); ``vp_std`` > 0 selects the
 * VP-SDE instead, with k->beta = beta(t) and vp_std = sigma_t (every other field of k is then ignored); vp_std = 0: PSLD.
 * State layout [B, 2c, hw] (PSLD: [x | m]) or [B, c, hw] (VP), NCHW, as everywhere in this section.  batch <= 65535.
 *
 * psld_rademacher_f32: out[i] = +-1 from the dropout hash of (seed, offset + i) - a function of those two numbers alone, so
 *   any split of a range into launches, and any launch geometry, writes the same values.
 * psld_pf_cotangent_f32: w = A^T z (f32) for the probe z (f32, the state's shape), A the linear map eps -> -1/2 g(t)^2 s(eps),
 *   s = -L_t^{-T} eps as psld_reverse_sde_f64 forms it:
 *     score_mode 0: w_x = 1/2 beta gamma c11 z_x + 1/2 beta M nu c21 z_m,  w_m = 1/2 beta gamma c12 z_x + 1/2 beta M nu c22 z_m
 *     score_mode 1: w = 1/2 beta M nu c22 z_m  [B, c, hw];   score_mode 2: w = 1/2 beta gamma c11 z_x  [B, c, hw]
 *     VP:           w = 1/2 beta / sigma_t z
 *   (products in f64, rounded to f32 once).  w has the shape of the network's output.
 * psld_pf_div_rhs_f64: with n = batch * 2c * hw (VP: batch * c * hw): out[0 : n] = F(u, t) = f - 1/2 g^2 s(eps_pred), the
 *   FORWARD-time probability-flow drift (= -f_bar of psld_reverse_sde_f64 / psld_vp_reverse_f64 with probability_flow, in
 *   their arithmetic); out[n + b] = div_lin + sum_i z_i vjp_i over sample b, div_lin = -1/2 beta (gamma + nu) c hw (VP:
 *   -1/2 beta c hw) the divergence of the linear drift, vjp = J_eps^T w (f32, the state's shape).  The sum is taken in f64
 *   in an order fixed by (c, hw) alone: bitwise repeatable, and a sample's value does not depend on the batch around it.
 *   out holds n + batch doubles: the right-hand side of the ODE on the augmented flat state [u, log-density increment].
 * psld_gauss_logp_f64: out[b] = log N(x_b; 0, var_x I) + log N(m_b; 0, var_m I) for u = [B, c_x + c_m, hw] f64 ([x | m];
 *   c_m = 0: x alone, the VP prior); f64, same fixed order.
 * workspace (the two reductions): >= psld_pf_workspace_bytes(batch) bytes. */
#define PSLD_PF_MAX_SLICES 32
long long psld_pf_workspace_bytes(int batch);
int psld_rademacher_f32(float* out, long long n, unsigned long long seed, unsigned long long offset,
                        hipStream_t stream);
int psld_pf_cotangent_f32(const float* z, const psld_em_coeffs_t* k, double vp_std, int batch, int c, int hw,
                          float* w, hipStream_t stream);
int psld_pf_div_rhs_f64(const double* u, const float* eps_pred, const float* vjp, const float* z,
                        const psld_em_coeffs_t* k, double vp_std, int batch, int c, int hw, double* out,
                        void* workspace, hipStream_t stream);
int psld_gauss_logp_f64(const double* u, double var_x, double var_m, int batch, int c_x, int c_m, int hw,
                        double* out, void* workspace, hipStream_t stream);
/* VP-SDE baseline (main/models/sde/vpsde.py:9-99): perturbation kernel and the reverse
 * drift / Euler-Maruyama update (mode 0: f_bar = -f + g^2*score; mode 1: x <- x + f_bar*dt + g*sqrt(dt)*z). */
/* ScoreLoss beyond the eps-MSE (main/losses.py:38-39, 55-63).  mode 1: L1 criterion, loss f32 = mean|sum |eps - eps_pred|;
 * mode 2: weighting 'nll', loss f64 = mean|sum (score(eps_pred) - score(eps))^2 * beta(t), score = -eps / std(t)
 * (vpsde.py:26-27, 97-99), t [batch] f64, per = C*H*W.  grad (optional): d loss / d eps_pred * grad_scale, f32.
 * workspace >= psld_reduce_workspace_bytes(batch*per). */
int psld_vp_score_loss(const float* eps, const float* eps_pred, const double* t, double beta0, double beta1,
                       int batch, long long per, int mode, int reduce_mean, void* loss, float* grad,
                       float grad_scale, void* workspace, hipStream_t stream);
/* Likelihood-weighted PSLD score loss (the composition of main/losses.py:55-63 with psld.py:230-260 and
 * :375-377, which the reference leaves as a TODO at losses.py:74).  coeffs: the table psld_perturb_coeffs_f64 wrote for this
 * very t [batch] (entries [8..10] = the covariance); the inverse-transpose coefficients of get_inv_coeff are formed from it
 * in f64 and cast to f32, the two scores and their difference e are f32 as in get_score, and
 *   loss (f64) = sum_b sample_weight_b * sum (beta(t_b) gamma e_x^2 + beta(t_b) M nu e_m^2)   [/ N for reduce_mean]
 * with N = batch*2c*hw in EVERY score mode (the element count of get_score's output, zero half included).
 * score_mode 0: eps, eps_pred, grad [B,2c,hw]; 1 (score_m, lower) / 2 (score_x, upper): eps_pred and grad [B,c,hw], the
 * target is the m / x half of eps [B,2c,hw].  sample_weight [batch] f64 or NULL (= 1).  grad (optional): d loss / d eps_pred
 * formed in f64, rounded to f32 once, times grad_scale.  The summation order is fixed by (batch, c, hw): bitwise repeatable.
 * workspace >= psld_reduce_workspace_bytes(batch*2*c*hw); batch <= 4096. */
int psld_nll_score_loss(const float* eps, const float* eps_pred, const double* t, const double* coeffs,
                        const double* sample_weight, const psld_sde_params_t* p, int score_mode, int batch, int c,
                        int hw, int reduce_mean, double* loss, float* grad, float grad_scale, void* workspace,
                        hipStream_t stream);
/* Importance-sampled training times: the inverse CDF at u [batch] (f64, in [0, 1)) of the piecewise
 * log-uniform density with masses mass [bins] (cum [bins + 1] their running sum, cum[0] = 0, cum[bins] = 1) on the bins
 * between exp(log_edges [bins + 1]):  k = the largest bin with cum[k] <= u,  r = (u - cum[k]) / mass[k],
 * t = clamp(exp(log_edges[k] + r * d_k), t_lo, t_hi), d_k = log_edges[k+1] - log_edges[k];
 * weight = 1 / (q(t) span) = t d_k / (mass[k] span), so that E_q[weight f(t)] = E_{U[t_lo, t_hi]}[f(t)] for span =
 * t_hi - t_lo.  Deterministic in u. */
int psld_sample_times_f64(const double* u, int batch, const double* cum, const double* log_edges, const double* mass,
                          int bins, double span, double t_lo, double t_hi, double* t, double* weight,
                          hipStream_t stream);
int psld_vp_perturb_f32(const float* x0, const float* eps, const double* t, double beta0, double beta1,
                        int batch, long long per_image, float* z_f32, double* u_f64, hipStream_t stream);
int psld_vp_reverse_f64(double* x, const float* eps_pred, const double* z, double beta, double std, double dt,
                        int probability_flow, int mode, long long n, double* f_bar, float* x_f32_out,
                        hipStream_t stream);
/* Classifier guidance (ClassCondEulerMaruyamaSampler.predictor_update_fn, samplers/sde.py:90-97): x += coef * grad
 * with coef_x on the position half and coef_m on the momentum half of the [B,2C,HW] f64 state (coef = g^2 * dt,
 * the classifier temperature already folded into grad); optionally refreshes the f32 copy. */
int psld_guide_f64(double* x, const float* grad, double coef_x, double coef_m, int batch, int c, int hw,
                   float* x_f32_out, hipStream_t stream);
/* Softmax cross entropy of [rows][n] logits vs int64 labels (nn.CrossEntropyLoss in PSLDTimeCELoss,
 * losses.py:147-173): *loss = loss_scale * sum_r (logsumexp(z_r) - z_r[y_r]); dlogits (optional) =
 * grad_scale * (softmax(z_r) - onehot(y_r)); *correct (optional) = number of rows whose argmax is the label. */
int psld_softmax_xent_f32(const float* logits, const long long* labels, int rows, int n, float loss_scale,
                          float grad_scale, float* loss, float* dlogits, float* correct, hipStream_t stream);
/* Inpainting combine (ES3EulerMaruyamaInpainter.inpaint_update_fn, samplers/sde.py:161-181): for the state
 * x = [x | m] and the re-perturbed known image u = [x_k | m_k], both [B,2C,HW] f64, x <- x*(1-mask) + u*mask with
 * mask [B,C,HW] f32 in {0,1} applied to both halves; optionally refreshes the f32 copy the network reads. */
int psld_mask_combine_f64(double* x, const double* u, const float* mask, int batch, int c, int hw,
                          float* x_f32_out, hipStream_t stream);
/* Class conditioning (model.score_fn.label_classes = K > 0; no counterpart in the reference, whose ncsnpp.py:288 leaves it as
 * a TODO).  table [n_rows = K + 1][d] f32 is NCSNpp.label_emb, row null_row = K the "no label" row; labels int64 [batch] in
 * [0, n_rows) (anything else is a contract violation the CALLER excludes: the add kernel skips such a sample, the gradient
 * kernel counts it for no row); drop (may be NULL) uint8 [batch]: non-zero -> the sample reads null_row instead of its label.
 * add:  temb[i][:] += table[lab_i][:] in place on the [batch][d] time embedding - one fp32 add per element.
 * grad: dtable[r][:] = sum_{i : lab_i = r} dtemb[i][:] for EVERY row r (rows nobody selects are written as zeros), summed in
 *       sample order without atomics (bitwise reproducible); accumulate != 0: dtable[r][:] += that sum. */
int psld_label_embed_add_f32(float* temb, const float* table, const long long* labels, const unsigned char* drop,
                             int batch, int d, int n_rows, int null_row, hipStream_t stream);
int psld_label_embed_grad_f32(const float* dtemb, const long long* labels, const unsigned char* drop, int batch, int d,
                              int n_rows, int null_row, float* dtable, int accumulate, hipStream_t stream);
/* Classifier-free guidance: eps2 [2n] f32 holds the conditional network output in [0, n) and the unconditional one in
 * [n, 2n); out[i] = u + scale * (c - u) (one subtraction, one fused multiply-add). */
int psld_cfg_combine_f32(const float* eps2, float scale, float* out, long long n, hipStream_t stream);
int psld_f64_to_f32(const double* x, float* y, long long n, hipStream_t stream);
int psld_f32_to_f64(const float* x, double* y, long long n, hipStream_t stream);

/* ---- per-step parameter maintenance over flat buffers (wrapper.py:82-89,128-155;
 *      callbacks.py:57-64): 97.6 M parameters in ONE launch each --------------------------------*/
/* norm_out[0] = sqrt(sum g^2) (double); workspace >= psld_reduce_workspace_bytes(n). */
int psld_grad_norm_f32(const float* g, long long n, double* norm_out, void* workspace, hipStream_t stream);
/* clip_coef = min(max_norm / (norm + 1e-6), 1) computed on device from norm_out (no host sync);
 * g *= clip_coef; Adam (torch.optim.Adam semantics, step is 1-based); optional EMA of p into ema.
 * max_norm <= 0 disables clipping (norm may be NULL).
 * err_word (may be NULL): a device error word of this step's backward (first 8 bytes of the team kernels' slot buffer,
 * psld_gn_bwd_team_f32): when it is non-zero at execution time the launch leaves p / m / v / ema untouched and writes NaN to
 * poison[0] (may be NULL; the loss scalar the caller logs) - bad gradients never reach the parameters, with no host read. */
int psld_adam_ema_f32(float* p, const float* g, float* m, float* v, float* ema, long long n,
                      const double* norm, double max_norm, double lr, double beta1, double beta2,
                      double eps, double weight_decay, int step, double ema_tau, int write_clipped_grad,
                      float* g_mut, const float* hyper_dev, const unsigned long long* err_word, float* poison,
                      hipStream_t stream);
/* The two per-step scalars of the kernel above, lr / (1 - beta1^step) and 1 / sqrt(1 - beta2^step), formed in
 * double like the launcher does: what a caller writes into hyper_dev[0..1] (device floats) before replaying a
 * captured training step (then lr / step of the captured call are ignored). */
void psld_adam_step_scalars(double lr, double beta1, double beta2, int step, float* out2_host);
/* The same two scalars written to a 2-float DEVICE buffer by a kernel that takes them by value (captured training step). */
int psld_adam_step_scalars_dev(double lr, double beta1, double beta2, int step, float* out2_dev, hipStream_t stream);
/* target = target*tau + src*(1-tau) (callbacks.py:62-64); hyper-parameters are doubles so that
 * (1 - tau), (1 - beta) are formed in double and rounded once, as torch does for python floats.
 * err_word as in psld_adam_ema_f32: non-zero -> no-op. */
int psld_ema_f32(float* target, const float* src, long long n, double tau, const unsigned long long* err_word,
                 hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PSLD_HIP_H */
