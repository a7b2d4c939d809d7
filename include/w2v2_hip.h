/*
 * w2v2_hip.h -- C ABI of libw2v2hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * wav2vec2 speaker-recognition training path of nikvaessen/w2v2-speaker.
 *
 * The reference has NO native / FFI interface: its seam is a set of torch
 * nn.Module contracts whose arithmetic lives in HuggingFace transformers / torch ATen.  Every entry
 * point below therefore cites the reference (or HF) call site whose device arithmetic it replaces:
 *   ref: = /root/reference/...      HF: = transformers/models/wav2vec2/modeling_wav2vec2.py (5.15.0)
 *
 * Conventions
 *   - plain C: pointers + sizes only, no torch types.  All pointers are DEVICE pointers unless the
 *     name ends in _host.  The caller owns every buffer (inputs, outputs, saved-for-backward,
 *     workspace); the library never allocates or frees device memory and keeps no pointer past a call.
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); no implicit sync.
 *   - return 0 on success, negative on error; w2v2_last_error() gives the message (thread local).
 *   - dtype codes: W2V2_F32 = 0, W2V2_BF16 = 1, W2V2_F16 = 2 (IEEE half: the precision of the reference's own
 *     fp16-AMP runs, config/experiment/speaker_wav2vec2_aam.yaml:17; its backward runs under the loss scale of
 *     w2v2_grad_scaler_*).  "act dtype" is the storage type of activations; statistics, reductions, biases,
 *     LayerNorm/GroupNorm parameters and gradients are always f32.
 *   - activations are channels-last: [B, T, C] row-major ("tokens x channels").
 */
#ifndef W2V2_HIP_H
#define W2V2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define W2V2_F32 0
#define W2V2_BF16 1
#define W2V2_F16 2

int w2v2_version(void);
const char* w2v2_last_error(void);

/* ------------------------------------------------------------------------------------------ GEMM
 * One tiled MFMA GEMM serves every matmul-shaped op of the path (HF:520-526 q/k/v_proj, HF:544
 * out_proj, HF:565-572 FFN, HF:429-435 projection, HF:254-272 conv layers 1-6 as implicit GEMM,
 * HF:326-368 grouped pos-conv as implicit GEMM, attention score / context products HF:438-463,
 * ref: src/optim/loss/aam_softmax.py:55 F.linear) and all of their backward products.
 *
 *   C[z][m][n] = epilogue( alpha * sum_k A[z](m,k) * B[z](n,k) )        z = 0..batch-1
 *
 * Operand storage: a 2-D array [outer][inner] with `inner` contiguous and outer stride `ld`
 * (elements).  trans = 0: outer = m (or n), inner = k.   trans = 1: outer = k, inner = m (or n).
 * The outer index may be segmented (implicit im2col of a strided conv over [B, L, C] activations):
 *   addr(outer) = (outer / seg_len) * seg_stride + (outer % seg_len) * ld      (seg_len = 0: plain)
 * Batch offsets are two-level: z -> (z / batch_inner, z % batch_inner) * (stride0, stride1).
 */
typedef struct {
  const void* ptr;
  int64_t ld;
  int64_t seg_len, seg_stride;
  int64_t stride0, stride1;
  int32_t trans;
  int32_t _pad;
} w2v2_operand;

enum {
  W2V2_EPI_NONE = 0,      /* C = alpha*acc                                              */
  W2V2_EPI_BIAS = 1,      /* C = alpha*acc + bias[n]                                    */
  W2V2_EPI_BIAS_GELU = 2, /* pre = alpha*acc + bias[n]; aux = pre (if aux); C = gelu(pre) */
  W2V2_EPI_GELU_BWD = 3,  /* C = alpha*acc * gelu'(aux[m][n])                           */
  W2V2_EPI_ADD = 4,       /* C = alpha*acc + aux[m][n]   (residual / gradient join)     */
  W2V2_EPI_SCALE_RC = 5,  /* C = alpha*acc * row_scale[m] * col_scale[n]  (AAM cosine)  */
  /* FFN pair of HF:565-572 with the activation derivative taken where the pre-activation is in f32 registers:
   * the forward product stores gelu'(pre) instead of pre (same bytes), the backward product multiplies by it
   * (1 VALU op per element instead of re-evaluating erf / exp on 30 M elements per layer) */
  W2V2_EPI_BIAS_GELU_GRAD = 6, /* pre = alpha*acc + bias[n]; aux = gelu'(pre); C = gelu(pre)   */
  W2V2_EPI_MUL = 7             /* C = alpha*acc * aux[m][n]                                    */
};

typedef struct {
  int32_t M, N, K;
  int32_t batch, batch_inner; /* batch_inner >= 1 */
  int32_t dtype_ab;           /* dtype of A and B                                        */
  int32_t dtype_c;            /* dtype of C and aux                                      */
  int32_t epilogue;
  w2v2_operand A, B;
  void* C;
  int64_t ldc, c_stride0, c_stride1;
  void* aux;
  int64_t ldaux, aux_stride0, aux_stride1;
  const float* bias;       /* [N] f32 (EPI_BIAS*)                                         */
  int64_t bias_stride1;    /* bias offset per (z % batch_inner)                           */
  const float* row_scale;  /* [M] f32, const float* col_scale [N] (EPI_SCALE_RC)          */
  const float* col_scale;
  float alpha;
  int32_t split_k;         /* >1: K split over grid.y, partial sums atomically ADDED into an
                              f32 C the caller zeroed (EPI_NONE only)                     */
  int32_t accumulate;      /* 1: C += result (f32 C, atomics; implied by split_k>1)       */
  int32_t _pad;
  /* Two-term weights (fp16 activations; 0 = off): B = B_hi + B_lo with B_lo = fp16(W - fp16(W)) stored
   * b_lo_offset ELEMENTS behind B_hi (same layout).  Output columns n >= n_ext_from run k_ext (= K) extra
   * K steps  sum_k A(m,k) * B_lo(n,k), i.e. C = A (B_hi + B_lo)^T with the weight rounding error of ~2^-22
   * instead of 2^-11.  Used for the value and output projections of the attention block, whose weight
   * rounding is the largest term of the embedding error budget (DESIGN.md "precision").  Runs on the 256x128
   * LDS-DMA ring kernel: plain NT product, K % 64 == 0, 16-byte aligned rows; anything else is an error. */
  int32_t k_ext, n_ext_from;
  int64_t b_lo_offset;
} w2v2_gemm_desc;

int w2v2_gemm(const w2v2_gemm_desc* d, void* stream);
/* Measurement hook (bench.py `roofline`): the same launch, timed by the dispatch's own begin / end timestamps
 * (hipExtLaunchKernelGGL with a start / stop event owned by the library, slot = index into its event pool) -- what
 * rocprofv3 reports for the kernel, without the ~3 us of dispatch time that two hipEventRecord calls around a launch
 * include.  Only products that run on the 256x128 ring or the phased 256x256 kernel (error otherwise).
 * w2v2_timer_read waits for slots [first_slot, first_slot + n) and writes their durations in milliseconds. */
int w2v2_gemm_timed(const w2v2_gemm_desc* d, void* stream, int slot);
int w2v2_timer_read(int first_slot, int n, float* ms_out);
/* The kernel family w2v2_gemm sends this descriptor to, from a dry run of the dispatch itself (nothing is launched):
 * 4 = phased 256x256, 2 = 256x128 ring, 1 = 128-row LDS-DMA, 3 = register-staged, 9 = exact f32 (register-staged,
 * csrc/gemm_f32.hip), 10 = exact f32 with LDS-DMA staging (csrc/gemm_f32_dma.hip); < 0 = rejected. */
int w2v2_gemm_kernel_of(const w2v2_gemm_desc* d);
/* Tuning hook (tools/gemm_shapes.py, not used by the training path): force the tile family of plain K-contiguous
 * 16-bit products -- 0 = the library's own dispatch, 1 = 128x128, 2 = 256x128 ring, 3 = 256x256x32 ring,
 * 4 = 256x256x64 phased.  Returns the previous setting. */
int w2v2_tune_gemm_kernel(int family);
/* Tools only (tools/gemm_attrib.py): time-attribution / placement variants of the 256x256x64 phased kernel for fp16
 * products -- bit 0 no DMA in the main loop, 1 no fragment reads, 2 no MFMAs, 3 no epilogue, bits 4-5 = DMA pieces of a
 * phase issued between its MFMAs, bit 6 / 7 plain / write-through epilogue stores.  Variants with bits 0-3 compute
 * garbage by design.  Returns the previous setting; 0 = the product kernel. */
int w2v2_tune_gemm_debug(int bits);
/* Tools only: force the kernel / block tile of the exact-f32 MFMA GEMM -- 0 = the library's choice; 1..4 = the
 * register-staged kernel (csrc/gemm_f32.hip) on 128x128 / 64x128 / 128x64 / 64x64; 11..15 = the LDS-DMA kernel
 * (csrc/gemm_f32_dma.hip) on (32 fi) x 128 tiles, fi = tile - 10; + 100 = the same with XCD-contiguous tile order.  A product the LDS-DMA kernel cannot take (segmented or
 * unaligned operands, K % 4 != 0, M or N <= 64) ignores codes >= 11.  Returns the previous setting. */
int w2v2_tune_gemm_f32_tile(int tile);
/* Tools only: time-attribution variants of the 256x128 ring GEMM's K loop (results are garbage) -- bit 0 no LDS-DMA pieces in
 * the steady-state loop, 1 no barrier, 2 no vmcnt wait, 3 no fragment reads.  Returns the previous setting; 0 = the product
 * kernel. */
int w2v2_tune_gemm_ring_debug(int bits);
/* Tools / tests: which kernel the LAST exact-f32 product ran on -- 0 = register-staged, else 10 fi + stages of the
 * LDS-DMA kernel (e.g. 52 = 160 x 128 tiles, two-stage ring); + 1000 = its time-attribution instantiation (tile codes
 * >= 200 of w2v2_tune_gemm_f32_tile, tools only: garbage results). */
int w2v2_gemm_f32_last_kernel(void);

/* Grouped weight-gradient GEMM (the backward of HF:520-526,544,565-572 nn.Linear weights/biases):
 *   dW_p[o][i] = sum_t dY_p[t][o] * X_p[t][i]      dbias_p[o] = sum_t dY_p[t][o]   (dbias may be NULL)
 * for 1..32 (dY, X) pairs in ONE launch, 16-bit operands [tokens][features] (K-major), f32 results
 * WRITTEN (not accumulated), no split-K, no atomics -> bitwise reproducible.
 * Contract: rows [tokens, tokens_padded) of every dY / X are readable and zero
 * (tokens_padded = tokens rounded up to 64); n_out, n_in multiples of 8; 16-byte aligned rows. */
typedef struct {
  const void* dY; int64_t ld_dy;
  const void* X;  int64_t ld_x;
  float* dW;      int64_t ld_dw;
  float* dbias;
  int32_t n_out, n_in;
} w2v2_wgrad_problem;
int w2v2_wgrad_grouped(const w2v2_wgrad_problem* problems, int n, int tokens, int tokens_padded,
                       int dtype /* W2V2_BF16 or W2V2_F16: element type of dY and X */, void* stream);
/* The kernel w2v2_wgrad_grouped sends these problems to, from a dry run of its routing itself (nothing is launched, no
 * operand pointer is read, only n_out / n_in): 1 = 128x128 two-stage, 2 = 256x128 ring, 3 = 256x256x32 ring,
 * 4 = 256x256x64 phased (also under the forced families 5 / 6); < 0 = n outside 1..32. */
int w2v2_wgrad_kernel_of(const w2v2_wgrad_problem* problems, int n);
/* Tools only (tools/gemm_shapes.py, tests): force the kernel of the grouped weight gradients -- 0 = the library's own
 * choice, 1 = 128x128 two-stage, 2 = 256x128 ring, 3 = 256x256x32 ring, 4 = 256x256x64 phased (5 / 6: with one / both DMA
 * pieces of a phase issued between its MFMAs).  Returns the previous value. */
int w2v2_tune_wgrad_kernel(int family);

/* ------------------------------------------------------------------------ conv feature extractor
 * Layer 0 of HF:382-419: Conv1d(1->C,k,stride,no bias) + GroupNorm(C groups == per-(b,c) over time,
 * biased var, eps) + GELU(erf)  (HF:302-323).  wav [B,N] f32 -> y [B,L,C] act dtype, channels-last.
 * Two passes, conv recomputed in both so the [B,L,C] pre-norm tensor never touches HBM:
 *   stats: per 128-frame chunk {mean, sum (u - mean)^2} from f64 accumulators -> partial[B][nchunk][C][2] (f32
 *          workspace of B * w2v2_conv0_workspace_floats() floats), combined in a fixed order (f64, pairwise-variance
 *          update: no E[u^2] - mean^2, exact on a constant waveform) into
 *          mean_rstd[B][C][2] = {mean, 1/sqrt(var+eps)}: deterministic and batch-invariant.
 *   apply: normalise + GELU + store. */
int w2v2_conv0_workspace_floats(int N, int C, int k, int stride);
int w2v2_conv0_stats(const float* wav, const float* w /*[C][k]*/, float* partial, float* mean_rstd,
                     int B, int N, int C, int k, int stride, float eps, void* stream);
/* Statistics for the matrix-core convolution that w2v2_conv0_apply uses for 16-bit outputs (x and w split into
 * bf16 hi+lo pairs, xh.wh + xh.wl + xl.wh in one K=32 MFMA, relative error ~2^-16); same arguments and
 * workspace as w2v2_conv0_stats, which it calls for shapes outside C % 128 == 0, 3k <= 32.
 * k == 10 (the wav2vec2 layer): NO convolution is run -- the conv is linear, so sum(y) and sum(y^2) over time are
 * w.S and w^T R w with the 10 + 55 window moments S[j] = sum_t x[t*stride+j], R[j][j'] = sum_t x[..+j] x[..+j'] of the
 * waveform (f64, fixed order: deterministic and batch-invariant); 16 us instead of 100 at B = 66, 3 s.
 * W2V2_CONV0_NO_GRAM=1 keeps the convolution-based statistics (A/B). */
int w2v2_conv0_stats_mfma(const float* wav, const float* w, float* partial, float* mean_rstd,
                          int B, int N, int C, int k, int stride, float eps, void* stream);
/* Variable-length batch (evaluation): frames = device int32[B], 1 <= frames[b] <= L, the valid conv-0 frames of each
 * utterance.  Statistics of utterance b over its first frames[b] frames only (chunks past the end skipped, the
 * straddling chunk counts its valid frames, the fold divides by frames[b]): bit-identical to the plain entry on the
 * utterance alone (B = 1, its own length), same workspace.  The _mfma form covers the window-moment path (k == 10);
 * its convolution-statistics branch (k != 10 or W2V2_CONV0_NO_GRAM) returns an error. */
int w2v2_conv0_stats_len(const float* wav, const float* w, float* partial, float* mean_rstd, const int* frames,
                         int B, int N, int C, int k, int stride, float eps, void* stream);
int w2v2_conv0_stats_mfma_len(const float* wav, const float* w, float* partial, float* mean_rstd, const int* frames,
                              int B, int N, int C, int k, int stride, float eps, void* stream);
int w2v2_conv0_apply(const float* wav, const float* w, const float* mean_rstd, const float* gamma,
                     const float* beta, void* y, int dtype, int B, int N, int C, int k, int stride,
                     void* stream);
/* Layer 0 of the feat_extract_norm="layer" family (HF:275-299; "-lv60" / xlsr checkpoints):
 * out[b, l, :] = GELU(LayerNorm_C(conv1d(wav, w [C][k], stride)[b, l, :] + bias)) -- the normalisation runs over the channels
 * of one frame (eps = nn.LayerNorm's default 1e-5 at the reference).  bias may be NULL (conv_bias=False).  f32 arithmetic,
 * `dtype` output; C % 8 == 0, C <= 512, k <= 16. */
int w2v2_conv0_layernorm_gelu(const float* wav, const float* w, const float* bias, const float* gamma, const float* beta,
                              void* out, int B, int N, int C, int k, int stride, float eps, int dtype, void* stream);
/* Backward of w2v2_conv0_layernorm_gelu (HF:275-299 layer 0, unfrozen feature extractor): from dy = dL/d(out) [B, L, C]
 * (`dtype`) it ADDS dw [C][k], dbias [C] (NULL when bias is NULL / not wanted), dgamma [C], dbeta [C] (f32).  The
 * convolution, bias and LayerNorm are recomputed from the waveform as the forward computes them; there is no data gradient.
 * The column sums leave the kernel as one partial row per workgroup in `workspace`
 * (w2v2_conv0_layernorm_gelu_bwd_workspace_floats(B, N, C, k, stride) floats) and are folded in a fixed order by a second
 * small launch: no atomics, bitwise the same in every run.  Same domain as the forward; outside it an error is returned
 * before any launch. */
int w2v2_conv0_layernorm_gelu_bwd_workspace_floats(int B, int N, int C, int k, int stride);
int w2v2_conv0_layernorm_gelu_bwd(const float* wav, const float* w, const float* bias, const float* gamma, const float* beta,
                                  const void* dy, float* dw, float* dbias, float* dgamma, float* dbeta, float* workspace,
                                  int B, int N, int C, int k, int stride, float eps, int dtype, void* stream);
/* Backward of layer 0 (unfrozen feature extractor): from dz = dL/d(layer-0 output) [B,L,C] compute dw [C][k],
 * dgamma [C], dbeta [C] (f32 atomics, caller zeroes); conv / GroupNorm are recomputed from the waveform and the
 * forward's mean_rstd.  sums [B][C][2] is f32 scratch. */
int w2v2_conv0_bwd(const float* wav, const float* w, const float* mean_rstd, const float* gamma,
                   const float* beta, const void* dz, float* sums, float* dw, float* dgamma, float* dbeta,
                   int dtype, int B, int N, int C, int k, int stride, void* stream);
/* col2im of a strided Conv1d data gradient: col [B*Lout][k*Cin] (= dpre @ packed weight) -> dx [B][Lin][Cin]. */
int w2v2_col2im(const void* col, void* dx, int B, int Lin, int Lout, int Cin, int k, int stride, int dtype,
                void* stream);
/* packed weight gradient [Cout][k][Cin] (f32) ADDED into the HF-layout gradient [Cout][Cin][k]. */
int w2v2_unpack_conv_grad(const float* gp, float* g, int Cout, int Cin, int k, void* stream);
/* HF conv weight [Cout][Cin][k] (f32) -> implicit-GEMM operand [Cout][k][Cin] (dtype). */
int w2v2_pack_conv_weight(const float* w, void* out, int dtype, int Cout, int Cin, int k, void* stream);

/* ----------------------------------------------------------------------------- LayerNorm family
 * y = LN(x + dropout(r)) * gamma + beta   (HF:429 feature_projection.layer_norm, HF:691-692 encoder
 * prologue, HF:596-601 post-LN residual blocks).  r may be NULL.  When r != NULL the pre-norm sum
 * s = x + dropout(r) is written back INTO r (saved for backward, no extra buffer).
 * Dropout (HF nn.Dropout) keeps element i when rand(seed, i) >= p and scales by 1/(1-p). */
int w2v2_layernorm_fwd(const void* x, void* r_inout, const float* gamma, const float* beta, void* y,
                       float* mean, float* rstd, int M, int H, float eps, float drop_p,
                       uint64_t seed, int dtype, void* stream);
/* y = GELU(LN(x) * gamma + beta), x and y [M, H] (y may alias x): the convolution layers of the feat_extract_norm="layer"
 * checkpoints (HF:275-299 Wav2Vec2LayerNormConvLayer: conv -> LayerNorm over the channels -> GELU).  No statistics are
 * saved: the backward recomputes them from x. */
int w2v2_layernorm_gelu_fwd(const void* x, const float* gamma, const float* beta, void* y, int M, int H, float eps,
                            int dtype, void* stream);
/* Backward of w2v2_layernorm_gelu_fwd (HF:275-299 layers 1-6, unfrozen feature extractor): dy and the saved pre-norm
 * z = conv + bias, both [M, H] in `dtype`; mean / rstd are recomputed from z.  Writes dz (may alias dy) and ADDS
 * dgamma, dbeta and dbias = sum_rows dz (the convolution's bias gradient; may be NULL) [H] f32.  The column sums leave
 * the kernel as one partial row per workgroup in `workspace` (w2v2_layernorm_gelu_bwd_workspace_floats(M, H) floats) and
 * are folded in a fixed order by a second small launch: no atomics, bitwise the same in every run.  H % 8 == 0, H <= 1024;
 * outside that an error is returned before any launch. */
int w2v2_layernorm_gelu_bwd_workspace_floats(int M, int H);
int w2v2_layernorm_gelu_bwd(const void* dy, const void* z, const float* gamma, const float* beta, void* dz, float* dgamma,
                            float* dbeta, float* dbias, float* workspace, int M, int H, float eps, int dtype, void* stream);
/* s = pre-norm input (x if r was NULL).  Outputs: ds (grad wrt s; may alias dy), d_r = ds*dropmask
 * (optional; a plain copy of ds when drop_p == 0), dgamma/dbeta ADDED to (f32, caller zeroes): with a
 * workspace of w2v2_layernorm_bwd_workspace_floats(H) floats the column sums are folded in a fixed
 * order by a second tiny kernel (deterministic, no atomics); workspace NULL falls back to f32 atomics. */
int w2v2_layernorm_bwd_workspace_floats(int H);
int w2v2_layernorm_bwd(const void* dy, const void* s, const float* mean, const float* rstd,
                       const float* gamma, void* ds, void* d_r, float* dgamma, float* dbeta,
                       float* workspace, int M, int H, float drop_p, uint64_t seed, int dtype,
                       void* stream);
/* Deferred fold: call w2v2_layernorm_bwd with dgamma = dbeta = NULL and a workspace -> the per-block column partials
 * stay in the workspace (one workspace per LayerNorm); this entry folds up to 8 of them (same M, H) into their
 * dgamma / dbeta (+=, fixed order) in ONE launch. */
typedef struct {
  const float* partial;    /* the workspace given to w2v2_layernorm_bwd */
  float* dgamma;
  float* dbeta;
} w2v2_ln_fold;
int w2v2_layernorm_bwd_fold(const w2v2_ln_fold* entries, int n, int M, int H, void* stream);

/* ---------------------------------------------------------------------------------- elementwise */
/* nn.Dropout fwd == bwd (same mask): y = x * keep(seed,i)/(1-p); in place allowed. */
int w2v2_dropout(const void* x, void* y, int64_t n, float p, uint64_t seed, int dtype, void* stream);
/* dx = dy * gelu'(pre)  (exact erf GELU, ACT2FN["gelu"]). */
int w2v2_gelu_bwd(const void* dy, const void* pre, void* dx, int64_t n, int dtype, void* stream);
/* Workspace rows of the fixed-order column reductions below: `partial` holds W2V2_PARTIAL_ROWS x (columns) f32; each
 * row block of the first pass WRITES one row, one w2v2_colsum row block then adds the rows to the target in a fixed
 * order (no atomics across blocks: the result is bitwise the same in every run). */
#define W2V2_PARTIAL_ROWS 256
/* dx[m][n] = dy * gelu'(pre) over a dense [M][N] matrix and colsum[n] += sum_m dx[m][n] (fixed order through `partial`,
 * caller zeroes): GELU backward of the positional convolution fused with its bias gradient (HF:360-368).  N % 8 == 0,
 * 16-byte aligned. */
int w2v2_gelu_bwd_colsum(const void* dy, const void* pre, void* dx, float* colsum, float* partial, int M, int N, int dtype,
                         void* stream);
/* y = x + a (gradient joins). */
int w2v2_add(const void* x, const void* a, void* y, int64_t n, int dtype, void* stream);
/* out[n] += sum_m x[m][n]   (bias gradients; f32 atomics, caller zeroes). */
int w2v2_colsum(const void* x, int64_t ld, float* out, int M, int N, int dtype, void* stream);
/* base[off_r .. off_r + n_r) = 0 for the (off, n) pairs of the int64 device table: gradient zeroing of the tensors the
 * backward ACCUMULATES into (LayerNorm gamma / beta, pos-conv bias, masked_spec_embed, LayerDrop-skipped layers) --
 * the large gradients are written, not accumulated (w2v2_wgrad_grouped), so the reference's optimizer.zero_grad()
 * (PL, torch.optim.Optimizer.zero_grad) does not have to touch them. */
int w2v2_zero_ranges(float* base, const int64_t* table, int n_ranges, int blocks_per_range, void* stream);
/* out[0] = mean of x[0..n): the scalar loss (ref: F.cross_entropy reduction="mean", aam_softmax.py:72). */
int w2v2_mean(const float* x, float* out, int n, void* stream);
/* f32 -> act dtype cast (bf16 weight copies), and strided 2-D copy/convert. */
int w2v2_cast(const float* x, void* y, int64_t n, int dtype, void* stream);
/* dst_i[C][R] = transpose(src_i[R][C]) for n matrices of one arena; table (device) holds per matrix
 * {src element offset, dst element offset, R, C}.  Refreshes the pre-transposed bf16 weight copies the
 * data-gradient GEMMs read (so dX = dY W runs K-contiguous like the forward products). */
int w2v2_transpose_many(const void* src, void* dst, const int64_t* table, int n, int blocks_per_matrix,
                        int dtype, void* stream);
/* SpecAugment time mask HF:1290-1292: h[m][:] = embed where mask[m].  Backward: d_embed += sum of
 * masked rows of dh (fixed order through `partial`, W2V2_PARTIAL_ROWS x H f32), masked rows of dh zeroed in place. */
int w2v2_mask_fill(void* h, const uint8_t* mask, const float* embed, int M, int H, int dtype,
                   void* stream);
/* SpecAugment feature mask HF:1294-1304 (`mask_feature_prob`, ref: config/network/wav2vec2_fc.yaml:56): h[b][t][c] = 0
 * where mask[b][c] (mask [B][H] bytes, 8-byte aligned, drawn on the host by the HF sampler AFTER the time mask).  The
 * backward is the same call on the gradient. */
int w2v2_mask_feature(void* h, const uint8_t* mask, int B, int T, int H, int dtype, void* stream);
int w2v2_mask_fill_bwd(void* dh, const uint8_t* mask, float* d_embed, float* partial, int M, int H, int dtype,
                       void* stream);
/* CLS token (ref: src/models/wav2vec2.py:128-140): y[b][0][:] = c, y[b][1+t][:] = x[b][t][:]. */
int w2v2_prepend_token(const void* x, void* y, float c, int B, int T, int H, int dtype, void* stream);
/* Paired-input sequence at per-pair lengths (ref: wav2vec2_paired_input.py:181-197): feat [R][H] row-major, y [B][T][H],
 * the four tables device int32[B].  With ta = left_frames[b], tb = right_frames[b]:
 *   y[b][0] = cls_c,  y[b][1 .. ta] = feat[left_row[b] ..],  y[b][ta+1] = sep_c,
 *   y[b][ta+2 .. ta+tb+1] = feat[right_row[b] ..],  y[b][ta+tb+2] = sep_c,  every later frame = 0.
 * Rows may be shared between pairs and come in any order; only named rows are read.  The caller guarantees
 * ta, tb >= 1, ta + tb + 3 <= T and both row ranges inside [0, R) (checked on the host before the tables are uploaded);
 * H % 8 == 0, T >= 5. */
int w2v2_pair_assemble(const void* feat, void* y, const int* left_row, const int* left_frames, const int* right_row,
                       const int* right_frames, float cls_c, float sep_c, int B, int T, int H, int dtype, void* stream);

/* ------------------------------------------------------------------------------------- pos-conv
 * HF:326-379 grouped weight-normed Conv1d(H,H,K,pad=K/2,groups=G) as an implicit GEMM per group:
 * regroup pads and splits channels  x [B,T,H] -> xg [B,G,T+K-1,H/G] (zero pad `pad_left` frames left).
 * weightnorm_pack: w = g*v/||v||_(per tap) -> fwd operand wf[G][co][tap][ci] and the flipped
 * operand wb[G][ci][K-1-tap][co] used by the data gradient; also returns inv norms.
 * weightnorm_bwd: from the packed weight gradient dwf[G][tap][ci][co] (f32; = the GEMM
 *   dwf_g[(tap,ci)][co] = sum_t xg_g[t][(tap,ci)] * dy_g[t][co], large dimension as M) -> dg[K],
 *   dv[H][H/G][K] (written, not added).
 * `sumsq` / `dot` are f32 scratch of w2v2_weightnorm_scratch_floats(H, G, K) = (1 + H)*K floats: [0,K) the per-tap
 * result, the rest per-block partials (one block per output channel) that are folded in a fixed order (bitwise
 * reproducible packed weights). */
int w2v2_posconv_regroup(const void* x, void* xg, int B, int T, int H, int G, int K, int pad_left,
                         int dtype, void* stream);
/* Variable-length batch: as w2v2_posconv_regroup, with frames t >= lens[b] (device int32[B], 1 <= lens[b] <= T)
 * written as zeros -- the zero padding Conv1d(padding = K/2) gives the utterance alone. */
int w2v2_posconv_regroup_len(const void* x, void* xg, const int* lens, int B, int T, int H, int G, int K, int pad_left,
                             int dtype, void* stream);
/* Weight gradient of the grouped positional conv as a correlation on the matrix cores (replaces the implicit-GEMM
 * call for 16-bit activations): dY [B*T, H] = gradient at the conv output (before the weight-norm), xg [B, G, T+K-1, H/G]
 * = posconv_regroup(x, pad_left = K/2); dwf [G][K*Cg][Cg] f32 is OVERWRITTEN (row (tap, ci), column co).
 * Cg = H/G in {16, 32, 48, 64}, K a multiple of 16.  (ref: the autograd of HF:360-368 `self.conv`.) */
int w2v2_posconv_wgrad(const void* dY, const void* xg, float* dwf, int B, int T, int H, int G, int K,
                       int dtype /* W2V2_BF16 or W2V2_F16 */, void* stream);
/* The grouped positional convolution itself (HF:326-379) and its data gradient as a DIRECT convolution with the padded
 * image of one (utterance, group) resident in LDS (csrc/posconv_direct.hip; w2v2-base geometry: Cg = 48, K = 128):
 *   out[b, t, g*Cg + co] = epi( sum_{tap, ci} xg[b, g, t + tap, ci] * w[g][co][tap*Cg + ci] )
 * xg = posconv_regroup(x, pad_left) [B][G][T+K-1][Cg]; w = the packed (weight-normed) weights [G][Cg][K*Cg] of
 * w2v2_weightnorm_pack (forward: wf; data gradient: wb over the regrouped dY).  mode 0: epi = GELU(. + bias[g*Cg+co]),
 * aux (may be NULL) receives the pre-activation; mode 1: epi = . + aux (aux may alias out).  16-bit activations;
 * bit-equal to the implicit GEMM of w2v2_gemm over the same operands.  Other geometries: use the implicit GEMM.
 * Contract: ldc a multiple of 8 elements; xg, w, out and aux 16-byte aligned (else an error is returned). */
int w2v2_posconv_direct(const void* xg, const void* w, void* out, void* aux, const float* bias, int B, int T, int G,
                        int Cg, int K, int64_t ldc, int mode, int dtype, void* stream);
int64_t w2v2_weightnorm_scratch_floats(int H, int G, int K);
int w2v2_weightnorm_pack(const float* g, const float* v, float* sumsq /*[(1+H)*K]*/, void* wf,
                         void* wb, int H, int G, int K, int dtype, void* stream);
int w2v2_weightnorm_bwd(const float* g, const float* v, const float* sumsq, const float* dwf,
                        float* dot /*[(1+H)*K]*/, float* dg, float* dv, int H, int G, int K,
                        void* stream);

/* ------------------------------------------------------------------------------------ attention
 * Unfused path (scores/context products go through w2v2_gemm): row softmax with dropout on the
 * probabilities (HF:455-457).  s [rows][T] f32 scores (already scaled by d^-1/2 via alpha),
 * p = softmax(s) (act dtype), p_drop = dropout(p) (only if drop_p > 0).
 * bwd: dS = P * (dP - sum(dP*P)) with dP = dPdrop*mask/(1-p); result f32 -> act dtype ds. */
int w2v2_softmax_fwd(const float* s, void* p, void* p_drop, int64_t rows, int T, int64_t ld,
                     float drop_p, uint64_t seed, int dtype, void* stream);
int w2v2_softmax_bwd(const float* dp_drop, const void* p, void* ds, int64_t rows, int T, int64_t ld,
                     float drop_p, uint64_t seed, int dtype, void* stream);
/* Variable-length batch, eval (no dropout): rows = B * heads * T; row r is query r % T of utterance r / (heads * T),
 * normalised over its keys < lens[b] (device int32[B], 1 <= lens[b] <= T), p = 0 for the other keys, all-zero rows
 * for queries >= lens[b].  Valid rows bit-identical to w2v2_softmax_fwd at T = lens[b]. */
int w2v2_softmax_fwd_len(const float* s, void* p, const int* lens, int B, int heads, int T, int64_t ld, int dtype,
                         void* stream);
/* Fused multi-head self-attention over QKV [B,T,3,heads,d] (HF:438-548 minus the projections),
 * one workgroup per (batch, head, query tile); saves row log-sum-exp for the backward.
 * ctx [B,T,heads*d].  bwd writes dqkv [B,T,3,heads,d]. */
int w2v2_attention_fwd(const void* qkv, void* ctx, float* lse, int B, int T, int heads, int d,
                       float scale, float drop_p, uint64_t seed, int dtype, void* stream);
int w2v2_attention_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse,
                       void* dqkv, float* delta /*[B,heads,T] scratch*/, int B, int T, int heads,
                       int d, float scale, float drop_p, uint64_t seed, int dtype, void* stream);
/* Variable-length batch, eval (no dropout): the fused forward with the per-utterance bound lens[b] (device int32[B],
 * 1 <= lens[b] <= T) in place of T; buffers keep the row stride of T.  Key / value rows >= lens[b] never enter the
 * arithmetic, ctx rows >= lens[b] are written as zeros, lse is written for rows < lens[b].  With the geometry forced
 * (W2V2_ATTN_GEOM), valid rows are bit-identical to w2v2_attention_fwd on the utterance alone at T = lens[b]. */
int w2v2_attention_fwd_len(const void* qkv, void* ctx, float* lse, const int* lens, int B, int T, int heads, int d,
                           float scale, int dtype, void* stream);

/* -------------------------------------------------------------------------------------- pooling
 * ref: src/layers/pooling.py:24-44,74-80,118-136.  x [B,T,H] act dtype -> out f32.
 * mode 0: mean+std  -> [B,2H] = cat(std_unbiased, mean)  (std FIRST, quirk Q1)
 * mode 1: mean      -> [B,H]       mode 2: max -> [B,H]
 * mode 3: first     -> [B,H]       mode 4: last / "middle" (quirk Q2) -> [B,H]
 * mode 5: quantile  -> [B,5H] = the 0 / .25 / .5 / .75 / 1 quantiles over time, quantile-major
 *         (ref: src/layers/pooling.py:51-67, torch.quantile with linear interpolation)
 * mode 16 + t: frame t -> [B,H]  (IndexPool1D "random", ref: src/layers/pooling.py:125-126,150-154: the HOST draws t
 *         with random.randint like the reference; NoPooling, :160-166, is the same call on the [B*T, 1, H] view) */
int w2v2_pool_fwd(const void* x, float* out, int B, int T, int H, int mode, int dtype, void* stream);
/* Variable-length batch: modes 0-5 over the first lens[b] frames (device int32[B], 1 <= lens[b] <= T) of each
 * utterance, rows strided by T; bit-identical to w2v2_pool_fwd on the [1, lens[b], H] slice. */
int w2v2_pool_fwd_len(const void* x, float* out, const int* lens, int B, int T, int H, int mode, int dtype,
                      void* stream);
/* dx [B,T,H] act dtype from dout f32 and the forward output (std/mean reused; max needs x). */
int w2v2_pool_bwd(const void* x, const float* out, const float* dout, void* dx, int B, int T, int H,
                  int mode, int dtype, void* stream);

/* ------------------------------------------------------------------- attentive statistics pooling
 * ref call site: src/layers/pooling.py:87-106 (AttentiveStatPool1D) -> speechbrain 0.5.x
 * AttentiveStatisticsPooling(C, attention_channels A = 128, global_context=True); speechbrain is not part of the
 * reference tree: the arithmetic follows its published definition (oracle.attentive_stat_pool).
 *   ctx [B][2C] = {mean_t x, std_t x} (biased, clamp 1e-12);  a = Wx x_t + (W1[:, C:] ctx + b1) (GEMM + cb);
 *   h = tanh(BatchNorm(relu(a))) with batch statistics over all B*T rows;  s = W2 h + b2 (GEMM);
 *   w = softmax_t s;  out [B][2C] = {sum_t w x, sqrt(clamp(sum_t w (x - mean)^2, 1e-12))}  (mean first).
 * x, a, h, s and their gradients are [B*T][.] act dtype; parameters / statistics f32.  The Wx / W2 products and
 * their data / weight gradients are w2v2_gemm / w2v2_wgrad_grouped calls made by the host. */
int w2v2_asp_context(const void* x, float* ctx, int B, int T, int C, int dtype, void* stream);
/* Variable-length batch (evaluation; ref call site as above, reached once per utterance by the batch-size-1 test loop of
 * src/lightning_modules/speaker/speaker_recognition_module.py:462-470): mean / std over the first lens[b] frames
 * (device int32[B], 1 <= lens[b] <= T) of each utterance, rows strided by T; bit-identical to w2v2_asp_context on the
 * [1, lens[b], C] slice. */
int w2v2_asp_context_len(const void* x, float* ctx, const int* lens, int B, int T, int C, int dtype, void* stream);
int w2v2_asp_context_bias(const float* ctx, const float* w1 /*[A][3C]*/, const float* b1, float* cb /*[B][A]*/,
                          int B, int A, int C, void* stream);
int w2v2_asp_bn_workspace_floats(int M, int A);
/* batch statistics of relu(a_pre) -> mean_rstd[A][2]; running = {mean[A], var[A]} updated like torch
 * BatchNorm1d (momentum, unbiased variance) or NULL */
int w2v2_asp_bn_stats(const void* a_pre, float* workspace, float* mean_rstd, float* running, int M, int A,
                      float eps, float momentum, int dtype, void* stream);
int w2v2_asp_bn_eval_stats(const float* running, float* mean_rstd, int A, float eps, void* stream);
int w2v2_asp_bn_tanh(const void* a_pre, const float* mean_rstd, const float* gamma, const float* beta, void* h,
                     int M, int A, int dtype, void* stream);
/* dh -> da_pre through tanh, BatchNorm (batch statistics) and relu; writes dgamma[A], dbeta[A].  tanh is
 * recomputed from a_pre (1 - h^2 from a stored bf16 h has no precision for saturated units). */
int w2v2_asp_bn_bwd(const void* dh, const void* a_pre, const float* mean_rstd, const float* gamma,
                    const float* beta, float* workspace, float* dgamma, float* dbeta, void* da, int M, int A,
                    int dtype, void* stream);
/* stats [B][C][2] = {max_t s, sum_t exp(s - max)} saved for the backward */
int w2v2_asp_pool_fwd(const void* x, const void* s, float* out, float* stats, int B, int T, int C, int dtype,
                      void* stream);
/* Variable-length batch (evaluation; same reference call site): softmax over the first lens[b] frames (device int32[B],
 * 1 <= lens[b] <= T) -- the scores of later frames enter neither the maximum, the sum nor the statistics (skipped, not
 * weighted by zero); bit-identical to w2v2_asp_pool_fwd on the [1, lens[b], C] slices of x and s. */
int w2v2_asp_pool_fwd_len(const void* x, const void* s, float* out, float* stats, const int* lens, int B, int T, int C,
                          int dtype, void* stream);
/* dout [B][2C] -> ds (through the softmax) and the direct part of dx (both written) */
int w2v2_asp_pool_bwd(const void* x, const void* s, const float* out, const float* stats, const float* dout,
                      void* ds, void* dx, int B, int T, int C, int dtype, void* stream);
/* context path: dW1[:, C:] (written), dx += d(mean, std) terms; scratch = B*A + B*2C floats */
int w2v2_asp_context_bwd(const void* x, const float* ctx, const void* da, const float* w1, float* dw1, void* dx,
                         float* scratch, int B, int T, int C, int A, int dtype, void* stream);

/* Paired-input head (ref: src/lightning_modules/speaker/wav2vec2_paired_input.py:200-206 nn.Linear(H,1) on the CLS
 * token + src/optim/loss/binary_cross_entropy.py:24-40): prob = sigmoid(emb.w + b), loss_rows = BCE-with-logits per
 * pair (mean taken by the caller); gradient outputs (all or none): dlogit[B] = (p-y)/B, demb[B][H], dw[H], db[1],
 * all multiplied by *loss_scale when that device pointer is given. */
int w2v2_bce_head_fwd_bwd(const float* emb, const float* w, const float* b, const int64_t* label, float* prob,
                          float* loss_rows, float* dlogit, float* demb, float* dw, float* db, int B, int H,
                          const float* loss_scale, void* stream);

/* Triplet margin head (ref: src/optim/loss/triplet_loss.py:21-107 -> F.triplet_margin_loss, p = 2, eps = 1e-6 added to
 * the difference, no swap; mean taken by the caller): emb [B][E] f32 with row stride ld; pos / neg [B] int64 (device)
 * name the positive and negative ROW of every anchor row.  d_ap / d_an [B] = ||a - p + eps|| / ||a - n + eps||,
 * loss_rows [B] = max(margin + d_ap - d_an, 0), unweighted.  demb [B][E] (contiguous; may be NULL: forward only)
 * = coef * *loss_scale / B * d(sum of loss rows)/d(emb), a row being active when margin + d_ap - d_an >= 0 (torch's
 * clamp_min backward); written when accumulate == 0 (rows nobody names and inactive rows: exact zeros), added to what
 * demb holds when accumulate != 0.  One writer per element and a fixed summation order (ascending anchor, its
 * positive term before its negative term): no atomics, bitwise reproducible.  An index outside [0, B) is not
 * dereferenced: NaN loss and distances for that row, no gradient.  d == 0 gives a zero unit vector.  Two launches. */
int w2v2_triplet_fwd_bwd(const float* emb, int64_t ld, const int64_t* pos, const int64_t* neg, float* d_ap,
                         float* d_an, float* loss_rows, float* demb, int B, int E, float margin, float coef,
                         int accumulate, const float* loss_scale, void* stream);

/* CTC loss on the device (ref: src/optim/loss/ctc_loss.py:36-58 -> F.ctc_loss(log_softmax(logits), blank,
 * reduction="mean", zero_infinity=True); src/lightning_modules/speaker/speaker_recognition_module.py:222-244).
 * logits [B*T][ldc] f32, utterance-major rows (row b * T + t), C classes of which `blank` is the blank.  targets: int64
 * (device), row b at targets + b * target_stride, `target_width` readable labels per row (0 <= width <= 31: the 2L + 1
 * <= 63 extended states of an utterance are one wavefront); the class of a label is label + target_offset (1 on the
 * speaker path, which leaves the caller's labels as they are; 0 for the generic loss).  input_lengths / target_lengths:
 * int32 [B] (device).  Outputs: loss_rows [B] = -log P(target | input) / max(L_b, 1), 0 where infinite (the mean over B
 * is the caller's); dlogits [B*T][ldc] in `dtype` (may be NULL: forward only, no gradient output is touched) =
 *   (softmax_t[c] - sum_{s: class(s) = c} gamma_t(s)) * *loss_scale / (B * max(L_b, 1))
 * for c < C (the padding columns are not written): exact zeros for the frames t >= input_lengths[b] and for every frame
 * of an utterance whose loss is infinite.  Repeated labels are merged before the subtraction; one writer per element, no
 * atomics, bitwise reproducible.  loss_scale (device pointer, may be NULL = 1) multiplies the gradient only.  A bad row --
 * a class outside [0, C) or equal to blank after the offset, a target length outside [0, target_width], an input length
 * outside [0, T] -- gives a NaN loss row and a zero gradient, and nothing out of range is read.  workspace: f32, 16-byte
 * aligned, at least w2v2_ctc_workspace_floats(B, T, target_width) elements (-1: bad arguments); the library allocates
 * nothing.  Three launches (two when forward only). */
int64_t w2v2_ctc_workspace_floats(int B, int T, int target_width);
int w2v2_ctc_fwd_bwd(const float* logits, int64_t ldc, const int64_t* targets, int64_t target_stride, int target_width,
                     int target_offset, const int* input_lengths, const int* target_lengths, int blank, float* loss_rows,
                     void* dlogits, const float* loss_scale, float* workspace, int64_t workspace_floats, int B, int T, int C,
                     int dtype, void* stream);

/* The same loss for transcripts (ref: src/lightning_modules/speech/speech_recognition_module.py:100-116): the contract
 * of w2v2_ctc_fwd_bwd word for word, with 0 <= target_width <= 1023.  The lattice of one utterance is one workgroup of
 * 64 ... 1024 threads (the smallest with target_width + 1 threads), thread j owning the blank state 2j and the label
 * state 2j + 1.  The workspace is laid out differently and is smaller per state (the posterior takes alpha's place, there
 * is no beta): at least w2v2_ctc_long_workspace_floats(B, T, target_width) elements (-1: bad arguments), 16-byte
 * aligned.  A bad row's part of the workspace is left as it was, apart from its status.  Three launches (two when
 * forward only).  w2v2_ctc_long_stage_frames: the number of frames whose emissions the lattice stages in LDS at a time
 * at this width (-1: bad width); the tests put utterance lengths around it. */
int64_t w2v2_ctc_long_workspace_floats(int B, int T, int target_width);
int w2v2_ctc_long_stage_frames(int target_width);
int w2v2_ctc_long_fwd_bwd(const float* logits, int64_t ldc, const int64_t* targets, int64_t target_stride, int target_width,
                          int target_offset, const int* input_lengths, const int* target_lengths, int blank,
                          float* loss_rows, void* dlogits, const float* loss_scale, float* workspace,
                          int64_t workspace_floats, int B, int T, int C, int dtype, void* stream);

/* Greedy CTC decoding (ref: speech_recognition_module.py:233-248, one argmax and one host synchronisation per utterance
 * there).  logits [B*T][ldc] f32 as above; per utterance b the argmax over c < C of every frame t < input_lengths[b] (the
 * lowest index wins a tie), runs of equal indices collapsed, THEN the blank dropped (`a a _ a` decodes to `a a`).
 * tokens_out int32 [B][T]: the first counts_out[b] entries of row b are the result in frame order, the rest is not
 * written; counts_out int32 [B] (-1 for an input length outside [0, T], of which nothing is read).  One launch, no
 * atomics; the caller copies tokens and counts to the host once per batch. */
int w2v2_ctc_greedy_decode(const float* logits, int64_t ldc, const int* input_lengths, int blank, int B, int T, int C,
                           int* tokens_out, int* counts_out, void* stream);

/* ------------------------------------------------------------------------------ ECAPA-TDNN pieces
 * ref: src/lightning_modules/speaker/ecapa_tdnn.py:75-85 -> speechbrain 0.5.x ECAPA_TDNN (not part of the reference
 * tree; restated in oracle/ecapa_oracle.py).  Channels-last [B*T][C] activations; `ld*` = row stride in elements so
 * Res2Net channel slices and the MFA concatenation are views of their parent tensors.
 * BatchNorm1d over the M rows of a channels-last [M][C] view (C, strides multiples of 8; of 4 for f32), on act(a):
 * act = W2V2_BN_ACT_NONE, W2V2_BN_ACT_RELU (ECAPA's TDNNBlock = conv -> ReLU -> BatchNorm) or W2V2_BN_ACT_LEAKY
 * (LeakyReLU with slope 0.01: the x-vector's conv -> LeakyReLU -> BatchNorm; the backward uses slope 0.01 at a == 0).  train = 1: batch statistics (biased variance) through `workspace`
 * partial sums, mean_rstd[C][2] written for the backward, running = {mean[C], var[C]} updated like torch or NULL;
 * train = 0: the running statistics (BatchNorm1d.eval()).  Two launches (partial sums, fold + apply), deterministic. */
#define W2V2_BN_ACT_NONE 0
#define W2V2_BN_ACT_RELU 1
#define W2V2_BN_ACT_LEAKY 2
int w2v2_bn_workspace_floats(int M, int C);
int w2v2_bn_fwd(const void* a, int64_t lda, float* workspace, float* mean_rstd, float* running, const float* gamma,
                const float* beta, void* y, int64_t ldy, int M, int C, float eps, float momentum, int act, int train,
                int dtype, void* stream);
/* dy -> da (through BatchNorm and the activation); writes dgamma[C], dbeta[C].  colsum_partial (may be NULL):
 * [w2v2_bn_colsum_rows(M, C)][C] f32, WRITTEN with the column sums of da over each row block -- the bias gradient of the
 * convolution in front of the BatchNorm (TDNNBlock = conv -> ReLU -> BatchNorm) is their sum: a w2v2_colsum over
 * M / 256 rows (M / 64 for the narrow Res2Net slices, whose row blocks are shorter so that they fill the chip) instead of
 * a second pass over the M rows of da. */
int w2v2_bn_colsum_rows(int M, int C);
int w2v2_bn_bwd(const void* dy, int64_t lddy, const void* a, int64_t lda, const float* mean_rstd, const float* gamma,
                float* workspace, float* dgamma, float* dbeta, void* da, int64_t ldda, int M, int C, int act,
                float* colsum_partial, int dtype, void* stream);
/* The same with the output gradient given as dy + dy2 (same shape, own row strides; both kernels add them as they read):
 * a Res2Net chunk's output feeds the next chunk and the block's concatenation, so its gradient has two sources. */
int w2v2_bn_bwd_sum(const void* dy, int64_t lddy, const void* dy2, int64_t lddy2, const void* a, int64_t lda,
                    const float* mean_rstd, const float* gamma, float* workspace, float* dgamma, float* dbeta, void* da,
                    int64_t ldda, int M, int C, int act, float* colsum_partial, int dtype, void* stream);
/* Conv1d(padding="same", padding_mode="reflect", dilation d, odd k) as im2col + GEMM:
 * col[(b,t)][j*Cin + c] = x[b][reflect(t + (j - (k-1)/2) d)][c]; col2im is its exact adjoint (gather, deterministic) */
int w2v2_im2col_reflect(const void* x, int64_t ldx, void* col, int B, int T, int Cin, int k, int dilation, int dtype,
                        void* stream);
/* The same over x + x2 (two row-strided operands of one shape, summed tap by tap): the input x_i + y_{i-1} of a Res2Net
 * chunk (speechbrain Res2NetBlock.forward) without a pass that materialises the sum. */
int w2v2_im2col_reflect_sum(const void* x, int64_t ldx, const void* x2, int64_t ldx2, void* col, int B, int T, int Cin,
                            int k, int dilation, int dtype, void* stream);
/* Variable-length batch (evaluation; ref: the batch-size-1 test loop of
 * src/lightning_modules/speaker/speaker_recognition_module.py:462-470 -> ecapa_tdnn.py:110-118 -> speechbrain
 * Conv1d(padding="same", padding_mode="reflect") on each utterance alone): lens = device
 * int32[B], dilation (k-1)/2 < lens[b] <= T (the caller checks on the host).  Taps reflect about the utterance's own last
 * frame lens[b] - 1; rows t >= lens[b] of col are written as zeros.  Rows t < lens[b] are bit-identical to
 * w2v2_im2col_reflect / _sum on the [1, lens[b], Cin] slice. */
int w2v2_im2col_reflect_len(const void* x, int64_t ldx, void* col, const int* lens, int B, int T, int Cin, int k,
                            int dilation, int dtype, void* stream);
int w2v2_im2col_reflect_sum_len(const void* x, int64_t ldx, const void* x2, int64_t ldx2, void* col, const int* lens,
                                int B, int T, int Cin, int k, int dilation, int dtype, void* stream);
int w2v2_col2im_reflect(const void* dcol, void* dx, int64_t lddx, int B, int T, int Cin, int k, int dilation,
                        int accumulate, int dtype, void* stream);
/* y[m][0..C) = a[m][0..C) + b[m][0..C) over row-strided views (Res2Net cumulative adds); b == NULL: y = a (a strided
 * copy: the pass-through chunk of a Res2Net block, the SE input slice). */
int w2v2_add_strided(const void* a, int64_t lda, const void* b, int64_t ldb, void* y, int64_t ldy, int M, int C,
                     int dtype, void* stream);
/* squeeze-excitation gate g [B][C] f32: y = x * g;  dg = sum_t dout * x;  dx = dout * g + ds / T */
int w2v2_se_scale(const void* x, const float* g, void* y, int B, int T, int C, int dtype, void* stream);
int w2v2_se_bwd_gate(const void* dout, const void* x, float* dg, int B, int T, int C, int dtype, void* stream);
int w2v2_se_bwd_x(const void* dout, const float* g, const float* ds, void* dx, int B, int T, int C, int dtype,
                  void* stream);
/* f32 vectors; mode 0 relu, 1 sigmoid; the backward takes the forward output */
int w2v2_act_fwd(const float* x, float* y, int64_t n, int mode, void* stream);
int w2v2_act_bwd(const float* dy, const float* y, float* dx, int64_t n, int mode, void* stream);

/* speechbrain StatisticsPooling of the x-vector over time: x f32 [B][T] rows of C channels (C % 4 == 0, row stride ldx,
 * T >= 2) -> out f32 [B][2C] = cat(mean, std_unbiased + eps), mean FIRST (w2v2_pool_fwd mode 0 has the std first and no
 * eps).  Two passes (mean, then centred squares), fixed-order reductions, no atomics.  stats [B][2C] (may be NULL)
 * receives (mean, std) for the backward.  _len: over the first lens[b] frames (device int32 [B], 2 <= lens[b] <= T) of
 * each utterance, bit-identical to the plain form on the [1, lens[b], C] slice.
 * bwd: dx[b][t][c] = dmean / T + dstd (x - mean) / ((T - 1) std), dout = cat(dmean, dstd); in a constant column
 * (std = 0) the second term is taken as 0, as torch's std backward does. */
int w2v2_stat_pool_fwd(const float* x, int64_t ldx, float* out, float* stats, int B, int T, int C, float eps,
                       void* stream);
int w2v2_stat_pool_fwd_len(const float* x, int64_t ldx, float* out, float* stats, const int* lens, int B, int T, int C,
                           float eps, void* stream);
int w2v2_stat_pool_bwd(const float* x, int64_t ldx, const float* stats, const float* dout, float* dx, int64_t lddx, int B,
                       int T, int C, void* stream);

/* ------------------------------------------------------------------------------------------------ wav2spk pieces
 * ref: src/lightning_modules/speaker/wav2spk.py:116-299, src/layers/temporal_gating.py.  f32 only, channels-last
 * [B*T][C] activations with a row stride; C, Cin and the row strides are multiples of 4 (one 16-byte vector per thread,
 * guards per vector).  No atomics, fixed-order reductions: bitwise reproducible.
 * `lens` (device int32 [B], may be NULL = every utterance has all T frames): the variable-length form of evaluation.
 * Every stage writes ZEROS into the rows at or past an utterance's own frame count, which is what lets the zero padding
 * of the next layer's gather fall out by itself; statistics blocks are counted from each utterance's first frame and do
 * not depend on T, so a row of a padded batch is bit-identical to the utterance run alone.
 *
 * Layer 0 (Cin = 1), straight from the waveform x [B] rows of N samples (row stride ldx):
 *   z[b][t][c] = bias[c] + sum_j w[c][j] * x[b][t * stride + j - pad], zero outside [0, n_b); T = (N + 2 pad - k) / stride + 1.
 *   lens here are SAMPLE counts n_b: utterance b has (n_b + 2 pad - k) / stride + 1 frames.
 * _bwd: dw[c][j] += sum_{b,t} dz[b][t][c] * x[b][t * stride + j - pad] through per-workgroup partial rows in `workspace`
 *   (w2v2_conv1d_first_bwd_workspace_floats of M = B * T rows) folded in block order in double.  No data gradient. */
int w2v2_conv1d_first(const float* x, int64_t ldx, const float* w, const float* bias, float* z, int64_t ldz, const int* lens,
                      int B, int N, int T, int C, int k, int stride, int pad, void* stream);
int w2v2_conv1d_first_bwd_workspace_floats(int M, int C, int k);
int w2v2_conv1d_first_bwd(const float* x, int64_t ldx, const float* dz, int64_t lddz, float* workspace, float* dw, int B,
                          int N, int T, int C, int k, int stride, int pad, void* stream);
/* Zero-padded strided gather: col[(b,t)][j * Cin + c] = x[b][t * stride + j - pad][c] or 0, Tout = (Tin + 2 pad - k) /
 * stride + 1, col rows contiguous (k * Cin); the convolution is this + a GEMM against the packed [Cout][k][Cin] weight.
 * col2im_zero is its exact adjoint written as a gather (dx WRITTEN, one writer per element, taps in ascending order). */
int w2v2_im2col_zero(const float* x, int64_t ldx, float* col, int B, int Tin, int Tout, int Cin, int k, int stride, int pad,
                     void* stream);
int w2v2_col2im_zero(const float* dcol, float* dx, int64_t lddx, int B, int Tin, int Tout, int Cin, int k, int stride,
                     int pad, void* stream);
/* y = relu(InstanceNorm1d(z)): no affine, no running statistics, biased variance over the frames of each (utterance,
 * channel).  Two launches per direction: per block of 128 frames the mean and the CENTRED second moment (sums in double:
 * a large DC component costs the variance nothing and a constant channel gives rstd = eps^-1/2 and y = 0 exactly), then
 * every workgroup combines the blocks of its utterance in double, in block order, and applies.  mean_rstd [B][C][2] is
 * written for the backward.  workspace: w2v2_instnorm_workspace_floats f32, shared by both directions.
 * _bwd: dz = rstd * (g - mean_t g - zhat * mean_t (g * zhat)), g = dy where y > 0 and 0 elsewhere, zhat = (z - mean) * rstd,
 * from the saved z, y and mean_rstd (training: fixed length only). */
int w2v2_instnorm_workspace_floats(int B, int T, int C);
int w2v2_instnorm_relu_fwd(const float* z, int64_t ldz, float* workspace, float* mean_rstd, float* y, int64_t ldy,
                           const int* lens, int B, int T, int C, float eps, void* stream);
int w2v2_instnorm_relu_bwd(const float* dy, int64_t lddy, const float* z, int64_t ldz, const float* y, int64_t ldy,
                           const float* mean_rstd, float* workspace, float* dz, int64_t lddz, int B, int T, int C,
                           void* stream);
/* Temporal gate over n contiguous elements (n % 4 == 0): y = sigmoid(p) * x with p = X W^T + b from a GEMM;
 * backward: dp = dy * x * s (1 - s) and the direct part dx = dy * s in one pass (the caller adds dp W). */
int w2v2_gate_fwd(const float* p, const float* x, float* y, int64_t n, void* stream);
int w2v2_gate_bwd(const float* dy, const float* p, const float* x, float* dp, float* dx, int64_t n, void* stream);
/* y[b][t][c] = act(bias[c] + ((p_0 + p_1) + ... + p_{S-1})[b][t][c]) over contiguous [B][T][C] rows, zeros for t >= lens[b]:
 * p_s = parts + s * part_stride are the partial products of a convolution whose K range was cut into S chunks (one batched
 * GEMM), folded in a fixed order; bias may be NULL, relu = 1 applies the aggregator's ReLU; y may be p_0. */
int w2v2_sum_bias_act_rows(const float* parts, int S, int64_t part_stride, const float* bias, float* y, const int* lens, int B,
                           int T, int C, int relu, void* stream);

/* ---------------------------------------------------------------------------------------- log-mel filterbank front-end
 * The ECAPA input features from waveforms (the device twin of data/fbank.py + InputNormalizer2D(True), data/pipeline.py;
 * ref: src/data/preprocess/audio_features.py:62-78, input_normalisation.py:44-75).  An utterance of n samples has
 * F = 1 + n / 160 frames; tap j in [0, 400) of frame t reads sample 160 t - 200 + j, zero outside [0, n) BY INDEX.
 * lens: device int32[B] SAMPLE counts (NULL: every utterance has N), 0 <= lens[b] <= N (clamped to that range).
 *
 * w2v2_fbank_db: wav [B][N] f32, window [400] (periodic Hamming), fbank [201][n_mels] -> db_out [B][T][n_mels] =
 * 10 log10(max(|DFT_400(window * frame)|^2 . fbank, 1e-10)) BEFORE the top-dB clamp, T = 1 + N / 160, and partial_max
 * [B][ceil(T / W2V2_FBANK_TILE_FRAMES)]: the maximum over tile i of frames [16 i, 16 i + 16) of the utterance (its own
 * frames only; tiles past F_b hold -inf, rows t >= F_b of db_out zeros).
 * w2v2_fbank_normalize: db = max(db, max over the utterance's F_b x n_mels cells - 80), then per mel channel over the
 * utterance's F_b frames (db - mean) / (std_unbiased + 1e-5) into out (row b T + t at out + (b T + t) ldo, n_mels
 * columns written, dtype W2V2_F32 or W2V2_BF16); rows t >= F_b are written as zeros.
 * Every cross-frame reduction runs in an order fixed by F_b alone: rows t < F_b of a padded batch are bit-identical to
 * the same two calls on the utterance alone (B = 1, N = n_b). */
#define W2V2_FBANK_TILE_FRAMES 16
int w2v2_fbank_db(const float* wav, const int* lens, const float* window, const float* fbank, float* db_out,
                  float* partial_max, int B, int N, int T, int n_mels, void* stream);
int w2v2_fbank_normalize(const float* db, const float* partial_max, const int* lens, void* out, int64_t ldo, int dtype,
                         int B, int T, int n_mels, void* stream);

/* ---------------------------------------------------------------------------------------- waveform augmentation (augment.hip, reverb.hip)
 * The `augmenter` stage of the reference's training pipelines (ref: src/data/preprocess/augment.py,
 * config/data/pipeline/xvector_*augment*.yaml: selector -> augmenter -> filterbank -> normalizer) on [B][N] f32 waveforms
 * that already live on the device, in front of w2v2_fbank_db.  The reference hands every chunk to WavAugment (libsox),
 * which is not available to compare against: THIS COMMENT IS THE DEFINITION of the six operations, its oracle is float64
 * numpy (tests/augment_cases.py); what was taken from memory of WavAugment is listed in DESIGN.md 7.  The random draws
 * (how many spans, where, which band, which speed, which SNR) are made on the host, in the reference's order of np.random
 * calls (data/augment.py); the kernels only take their results as small device tables.
 *
 * Shared conventions.  Everything is f32.  A buffer is [rows][ld] with N valid columns, ld >= N, every row * ld formed in
 * 64 bits.  Every entry takes a device int32 row list of R entries and touches only the rows it names (a row named twice
 * is the caller's error); every other row, and every column >= N, keeps its bits.  Per-row parameter tables are indexed by
 * the POSITION r in the list.  lens: device int32 sample counts indexed by the ROW NUMBER of the buffer that is read (NULL:
 * every row has N), clamped to [0, N]; samples at index >= lens[b] count as zero BY INDEX whatever the buffer holds, and
 * columns [len, N) of a touched row are written as zeros.  A row's result is a function of that row's own samples and
 * parameters alone, each output accumulated in one fixed order: it is bit-identical to the same call on the row alone
 * (R = 1, any B, any N >= len).  No atomics, one writer per element, nothing allocated, all work on `stream`.
 *
 * time dropout (in place): spans [R][S][2] int32 = (start, length) per listed row; x[start .. start + length) = 0, clipped
 * to [0, len).  length <= 0 is a no-op, spans may overlap, S = 0 only zeroes the columns behind len. */
int w2v2_aug_time_dropout(float* x, int64_t ld, int N, const int32_t* lens, const int32_t* rows, int R,
                          const int32_t* spans, int S, void* stream);
/* additive noise (in place): y[i] = fma(c, x[i], (1 - c) u[i]) for i < len, c = coef[r] f32 (1 - c formed in f32).  With
 * the SNR in dB, r = 10^(snr / 10) and c = r / (1 + r) on the host.
 * mix_uniform: u[i] in [0, 1) = (h >> 8) 2^-24 with h = rng_pair(rng_key(((uint64) row << 32) | rng_key(seed)), i), the
 * counter hash of csrc/common.h (dropout's), keyed by the seed, the ROW NUMBER and the sample index: the same seed gives
 * the same stream again, two rows under one seed get different streams.  The uniform [0, 1) law of the reference's
 * torch.zeros_like(x).uniform_() -- DC offset of 1/2 included -- but not its bit stream. */
int w2v2_aug_mix_uniform(float* x, int64_t ld, int N, const int32_t* lens, const int32_t* rows, int R, const float* coef,
                         int64_t seed, void* stream);
/* mix_bank: u[i] = bank[bank_row[r]][i mod bank_lens[bank_row[r]]], bank [M][ld_bank] f32 on the device: the noise
 * repeated until it covers the utterance, then cut (ref: augment.py:374-392).  A bank row outside [0, M) or a bank
 * length outside [1, ld_bank] is not dereferenced: that row's samples come out NaN. */
int w2v2_aug_mix_bank(float* x, int64_t ld, int N, const int32_t* lens, const int32_t* rows, int R, const float* coef,
                      const float* bank, int64_t ld_bank, const int32_t* bank_lens, int M, const int32_t* bank_row,
                      void* stream);
/* FIR, zero-phase "same" alignment (src row src_rows[r] -> dst row dst_rows[r]; the two buffers must not overlap):
 *   y[n] = sum_{j = 0}^{K - 1} h[j] x[n + (K - 1) / 2 - j],   0 <= n < min(len, N_out),   x zero outside [0, len)
 * with h = taps[r][0 .. K), K = ntaps[r] odd, 1 <= K <= W2V2_AUG_MAX_TAPS <= ldt; rows of one launch may differ in K.
 * len = clamp(lens[src_rows[r]], 0, N_in); columns [len, N_out) of the dst row are zeros, a row longer than N_out is
 * cropped.  Each output is one chain of f32 fmas over j = K - 1 down to 0 (every tap, also those that meet a zero by
 * index).  A bad tap count is not run: that dst row comes out NaN.  One workgroup per (row, tile of w2v2_aug_fir_tile()
 * outputs): the tile plus its halo and the reversed taps are staged in LDS, a thread keeps 8 consecutive outputs in
 * registers and slides a 12-sample window over the taps, 32 fmas per two 16-byte LDS reads. */
#define W2V2_AUG_MAX_TAPS 2561
int w2v2_aug_fir_tile(void);
int w2v2_aug_fir(const float* src, int64_t ld_src, int N_in, const int32_t* lens, const int32_t* src_rows, float* dst,
                 int64_t ld_dst, int N_out, const int32_t* dst_rows, int R, const float* taps, int64_t ldt,
                 const int32_t* ntaps, void* stream);
/* Rational resampling by U / D (speed 1 / (U / D) followed by a return to the sample rate), one launch per ratio over
 * the rows of that ratio; h [2 half + 1] is the prototype low-pass at the U-times-oversampled rate (data/augment.py designs
 * it: Kaiser-windowed sinc, cutoff 1 / max(U, D), half = 32 max(U, D)):
 *   out_len = min(ceil(len U / D), N_out),   y[m] = U * sum_j x[j] h[m D - j U + half],   0 <= m < out_len
 * over the j in [0, len) whose tap index lies in [0, 2 half], ascending j, one chain of f32 fmas, then one multiply by U.
 * Columns [out_len, N_out) are zeros; out_lens[dst_rows[r]] = out_len (out_lens may be NULL).  U == D copies the row
 * (bit-exact, h is not read).  1 <= U, D <= 4096, 0 <= half <= 2^20. */
int w2v2_aug_resample_tile(void);
int w2v2_aug_resample(const float* src, int64_t ld_src, int N_in, const int32_t* lens, const int32_t* src_rows, float* dst,
                      int64_t ld_dst, int N_out, const int32_t* dst_rows, int32_t* out_lens, int R, int U, int D,
                      const float* h, int half, void* stream);
/* Reverb (reverb.hip; src row src_rows[r] -> dst row dst_rows[r], the two buffers must not overlap): sox's `reverb
 * <reverberance> <damping> <room scale>` followed by `channels 1`, the freeverb bank of 8 damped feedback combs and 4
 * all-passes per output channel, restated from memory of sox's reverb.c.  The host (data/augment.py
 * reverb_parameters) does this arithmetic in float64:
 *   comb lengths at 44.1 kHz {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617}, all-pass {225, 341, 441, 556}, stereo
 *   adjust 12.  A mono input at sox's default stereo depth of 100 gives two filter arrays w = 0, 1.  r = rate / 44100,
 *   scale = room_scale / 100 * 0.9 + 0.1; a sign s starts at +1 and flips after every filter, through the 8 combs and on
 *   through the 4 all-passes; comb i has the delay int(scale r (comb[i] + 12 s w) + 0.5), all-pass j the delay
 *   int(r (allpass[j] + 12 s w) + 0.5) (no scale).  a = -1 / ln(0.7), b = 100 / (ln(0.02) a + 1),
 *   feedback = 1 - exp((reverberance - b) / (a b)), damp = damping / 100 * 0.3 + 0.2, wet_gain = 0.015 (0 dB, no pre-delay).
 * and hands the kernel one row of W2V2_AUG_REVERB_PARAMS int32 per listed row, indexed by the position r: comb delays
 * [w * 8 + i] at 0 .. 15, all-pass delays [w * 4 + j] at 16 .. 23, then the bits of the f32 feedback, damp, wet_gain and
 * dry_gain.  In exact arithmetic, for n < len = clamp(lens[src_rows[r]], 0, N_in), x zero by index outside [0, len):
 *   comb (a line of `delay` zeros, store = 0):  o = line[p];  store = o + (store - o) damp;  line[p] = x[n] + store feedback;
 *                                               the output is o; p advances round the line
 *   array w:  acc = 0, acc += comb_i(x[n]) for i = 7 down to 0;  then all-pass j = 3 down to 0, each
 *             o = line[p], line[p] = in + 0.5 o, out = o - in;   wet_w[n] = out wet_gain
 *   y[n] = 0.5 ((dry_gain x[n] + wet_0[n]) + (dry_gain x[n] + wet_1[n]))
 * dry_gain = 1 is the reference, dry_gain = 0 the wet signal alone.  The length is unchanged (no drain); columns
 * [len, N_out) of the dst row are zeros, a row longer than N_out is cropped.  sox's conversion to 32-bit integer samples
 * and its clipping at +-1 between effects are left out.
 * In f32 the low-pass `store` is evaluated as a scan over blocks of up to 64 samples with the carried store folded in
 * (reverb.hip states the order), so the result is defined to a tolerance against the sequential loop, not bit for bit;
 * the order is a function of the row's own table and length alone: a row is bit-identical to the same call on the row
 * alone, and a repeated launch is bit-identical.  Every delay must lie in [1, W2V2_AUG_REVERB_MAX_DELAY]: enough for every
 * room scale up to a sample rate of 27,940 Hz (at 32 kHz up to room scale 85, at 44.1 kHz up to 59).  A row with a delay
 * outside that range is not run: its dst row comes out NaN.  One workgroup walks one row in time chunks of
 * w2v2_aug_reverb_chunk() samples with the 24 delay lines in LDS; no workgroup waits on another, no workspace. */
#define W2V2_AUG_REVERB_MAX_DELAY 1024
#define W2V2_AUG_REVERB_PARAMS 28
int w2v2_aug_reverb_chunk(void);
int w2v2_aug_reverb(const float* src, int64_t ld_src, int N_in, const int32_t* lens, const int32_t* src_rows, float* dst,
                    int64_t ld_dst, int N_out, const int32_t* dst_rows, int R, const int32_t* params, void* stream);

/* ---------------------------------------------------------------------------------------- skinny linear layers
 * Exact-f32 nn.Linear / Conv1d(k=1) over a handful of rows (one per utterance): the SE bottleneck and the embedding
 * layer of ECAPA (speechbrain SEBlock / ECAPA_TDNN.fc) and the hidden fc_list of the wav2vec2 head (ref:
 * src/lightning_modules/speaker/wav2vec2_fc.py:108-141).  x [B][K], W [N][K], y [B][N] row-major, K % 4 == 0.
 * act: 0 none, 1 relu, 2 sigmoid.  fwd: y = act(x W^T + bias).  The backward entries take the forward OUTPUT y and
 * use dy' = dy * act'(y):  bwd_x: dx = dy' W;  bwd_w: dW (+)= dy'^T x, dbias (+)= column sums of dy' (dbias may be
 * NULL). */
int w2v2_skinny_linear_fwd(const float* x, const float* W, const float* bias, float* y, int B, int N, int K, int act,
                           void* stream);
int w2v2_skinny_linear_bwd_x(const float* dy, const float* y, const float* W, float* dx, int B, int N, int K, int act,
                             void* stream);
int w2v2_skinny_linear_bwd_w(const float* dy, const float* y, const float* x, float* dW, float* dbias, int B, int N,
                             int K, int act, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------- heads
 * Row inverse L2 norms 1/max(||x||,1e-12) (F.normalize, ref: src/optim/loss/aam_softmax.py:55). */
int w2v2_row_invnorm(const void* x, int64_t ld, float* inv, int rows, int cols, int dtype,
                     void* stream);
/* AAM margin + scale + softmax + CE (ref: aam_softmax.py:57-72) on cos [B][ldc] f32 (in: cosine).
 * margin < 0 selects the plain CE head (ref: src/optim/loss/cross_entropy.py:27-31; `cos` holds
 * logits, scale ignored).  Outputs: softmax [B][ldc] f32, loss_rows [B] f32 (mean is the caller's),
 * and for the backward, with g = dLoss/dcos (loss = mean over B):
 *   dcos_w[b][c] = g * inv_w[c]   (A operand of the embedding-gradient GEMM; inv_w NULL -> g)
 *   dcos_x[b][c] = g * inv_x[b]   (A operand of the weight-gradient GEMM;    inv_x NULL -> g)
 *   rowdot[b] = sum_c g*cos,  colprod[b][c] = g*cos ([B][C] f32, row stride C: the caller folds the rows in a fixed
 *   order -- w2v2_colsum with B <= 128 has one writer per column -- into coldot[c] = sum_b g*cos for
 *   w2v2_normalize_bwd; no atomics, so the head's weight gradient is bitwise reproducible); any may be NULL.
 * loss_scale (device pointer, may be NULL = 1): g is multiplied by *loss_scale (w2v2_grad_scaler_*); the loss
 * rows and the softmax are never scaled.  Labels outside [0, C) give loss = NaN for that row and zero gradients.
 * correct_rows [B] (may be NULL): 1 if argmax_c softmax[b][c] == label[b] else 0 -- the reference's train_acc
 * (ref: src/lightning_modules/speaker/speaker_recognition_module.py:296-307). */
int w2v2_aam_softmax_fwd_bwd(const float* cos, const int64_t* label, float* softmax,
                             float* loss_rows, void* dcos_w, void* dcos_x, const float* inv_x,
                             const float* inv_w, float* rowdot, float* colprod, int B, int C,
                             int64_t ldc, float margin, float scale, const float* loss_scale,
                             float* correct_rows, int easy_margin /* ref: aam_softmax.py:60-61 */, int dtype, void* stream);
/* Margin heads: sub-centres, the additive cosine margin and the inter-top-k penalty in one row pass.  These semantics
 * are DEFINED HERE (no reference file has such a head; the oracle of the tests is float64 torch).
 * cos [B][ld] f32 holds the cosines of C classes x K sub-centres, sub-centre k of class c in column c*K + k
 * (1 <= K <= 8, ld >= C*K; columns [C*K, ld) are never read).  One row b with label y:
 *   m_c = max_k cos[c*K + k], k*_c the smallest k that attains it;
 *   label logit: W2V2_MARGIN_ARC: phi(m_y) as w2v2_aam_softmax_fwd_bwd (hard threshold or easy_margin);
 *                W2V2_MARGIN_COS: phi = m_y - margin, dphi = 1 (easy_margin ignored);
 *   inter-top-k: the n_top classes c != y with the largest m_c (ties: the smaller class index; the label column is never
 *     a candidate) get psi = m_c cos(inter_margin) + sqrt(clamp(1 - m_c^2, 0, 1)) sin(inter_margin),
 *     dpsi = cos(inter_margin) - sin(inter_margin) m_c / max(sine, 1e-12);  0 <= n_top <= min(C - 1, 16);
 *   every other class z_c = m_c; all logits times `scale`; loss row = lse(z) - z_y.
 * softmax [B][ldp] f32 over the C CLASSES (ldp >= C); correct_rows[b] = 1 when the first arg-max class is the label.
 * Gradient g_c = dLoss/dm_c * loss_scale / B (dphi / dpsi included) goes to column c*K + k*_c alone; the other K - 1
 * columns of the class get exact zeros in dcos_w, dcos_x and colprod:  dcos_w = g * inv_w[column], dcos_x = g * inv_x[b],
 * colprod = g * cos ([B][C*K] f32, row stride C*K), rowdot[b] = sum g * cos.  The pointers loss_scale, inv_x, inv_w,
 * dcos_w, dcos_x, rowdot, colprod and correct_rows follow the null conventions of w2v2_aam_softmax_fwd_bwd; a label outside
 * [0, C): NaN loss row, zero gradients, correct 0.  No atomics, one writer per element, fixed-order folds; with K = 1,
 * n_top = 0 and W2V2_MARGIN_ARC every output has the bits of w2v2_aam_softmax_fwd_bwd. */
#define W2V2_MARGIN_ARC 0
#define W2V2_MARGIN_COS 1
int w2v2_margin_softmax_fwd_bwd(const float* cos, const int64_t* label, float* softmax, float* loss_rows,
                                void* dcos_w, void* dcos_x, const float* inv_x, const float* inv_w,
                                float* rowdot, float* colprod, int B, int C, int K, int64_t ld, int64_t ldp,
                                float margin, float scale, int easy_margin, int margin_type, int n_top,
                                float inter_margin, const float* loss_scale, float* correct_rows, int dtype,
                                void* stream);
/* F.normalize backward: dx = inv[r] * (g[r] - x[r] * inv[r] * dot[r]);  g, dx f32 (dx written or
 * added), x f32 or act dtype. */
int w2v2_normalize_bwd(const float* g, const void* x, int64_t ldx, const float* inv,
                       const float* dot, float* dx, int rows, int cols, int x_dtype, int add,
                       void* stream);
/* Class-weight gradient of the AAM head in one launch (ref: the autograd of src/optim/loss/aam_softmax.py:55 through
 * F.normalize(W)): dW[c][e] = inv_w[c] * (sum_b dcos_x[b][c] * emb[b][e] - W[c][e] * inv_w[c] * sum_b colprod[b][c]).
 * dcos_x [B][ldc] and emb [B][E] in `dtype` (the head's 16-bit operands, or f32), colprod [B][C] f32 = g * cos per element
 * (w2v2_aam_softmax_fwd_bwd), W [C][E] f32 master weights, dW [C][E] f32 WRITTEN.  E % 8 == 0, 16-byte aligned operands;
 * fixed summation order. */
int w2v2_aam_dw(const void* dcos_x, int64_t ldc, const void* emb, const float* colprod, const float* W,
                const float* inv_w, float* dW, int B, int C, int E, int dtype, void* stream);

/* ---------------------------------------------------------------------------------- trial scoring
 * The last stage of the speaker path on device buffers: f32 banks with D % 4 == 0 and row stride ld >= D (elements,
 * ld % 4 == 0, 16-byte aligned base); every row * ld is formed in 64 bits.  No atomics, fixed-order folds: equal inputs
 * give equal bits.  Nothing is allocated; all work goes on `stream`.
 *
 * Per-dimension mean and UNBIASED std over the N rows of bank [N][ld] -> mean_out / std_out [D] (ref:
 * speaker_recognition_evaluator.py:154-159 compute_mean_std_batch, called by CosineDistanceEvaluator.fit_parameters at
 * cosine_distance.py:84-97).  Per chunk of 128 rows the mean and the CENTRED second moment, summed in double; the chunks
 * are combined in double in chunk order (E[x^2] - mean^2 is never formed: a constant dimension gives std exactly 0).
 * workspace: caller-owned, 2 * ceil(N / 128) * D doubles, 8-byte aligned.  Two launches.  N < 2 is an argument error. */
int w2v2_embed_stats(const float* bank, int64_t ld, int N, int D, float* mean_out, float* std_out, void* workspace,
                     void* stream);
/* Cosine score of P trials over bank [N][ld]; pairs [P][2] int32 (device) names the two rows of each trial (ref:
 * cosine_distance.py:105-132 _compute_prediction_scores + :235-241 compute_cosine_scores, which stack a left and a right
 * [P][D] tensor on the host).  One trial per wavefront, one pass over the two rows.  With mean / std [D] (both NULL or both
 * set) every element is first u = (x - mean) / (std + 1e-12) in f32 (center_batch, speaker_recognition_evaluator.py:162-167);
 * with length_norm != 0 the rows are rescaled by 1 / max(||u||, 1e-12) (F.normalize; the three sums rescale, no second
 * pass); then cos = a.b / (max(||a||, 1e-8) * max(||b||, 1e-8)), each norm clamped on its own as torch's
 * cosine_similarity does.  cos_out [P] = cos, score_out [P] = clamp((cos + 1) / 2, 0, 1) (speaker_recognition_evaluator.py:81).
 * An index outside [0, N) is not dereferenced: both outputs of that trial are NaN. */
int w2v2_score_pairs(const float* bank, int64_t ld, int N, int D, const int32_t* pairs /*int32 [P][2]*/, int P,
                     const float* mean, const float* std /*both null or both set*/, int length_norm, float* cos_out /*[P]*/,
                     float* score_out /*[P]*/, void* stream);
/* The non-pooled score (ref: cosine_distance.py:187-232 compute_non_pooled_cosine_scores: per trial two [<= 50][D] frame
 * tensors, 2500 cosines and their mean, in a Python loop).  frames [rows][ld] is a ragged frame bank; sel [P][2][W] int32
 * holds ABSOLUTE row numbers, counts [P][2] int32 how many of the W slots of each side are used (1 <= W <= 256).  Uses
 *   mean_{i,j} cos(l_i, r_j) = < mean_i l_i / max(||l_i||, 1e-8) , mean_j r_j / max(||r_j||, 1e-8) >,
 * exact because the two norms are clamped separately: count_l + count_r row reads (each row twice) and one D-length dot
 * per trial.  One workgroup per trial; every wave folds its rows in ascending position, the waves are folded in wave
 * order; sums in double.  A count outside [1, W] or a selected row outside [0, rows) gives NaN outputs without a frame
 * read.  No centring and no length norm, as in the reference. */
int w2v2_score_frame_sets(const float* frames, int64_t ld, int64_t rows, int D,
                          const int32_t* sel /*int32 [P][2][W]: absolute row numbers*/, const int32_t* counts /*int32 [P][2]*/,
                          int W, int P, float* cos_out, float* score_out, void* stream);

/* ---------------------------------------------------------------------------------- score normalisation (score_norm.hip)
 * Adaptive score normalisation with a cohort (Z-, T- and S-norm; K = M gives the non-adaptive forms), between the scores
 * above and the metrics below.  The project this one mirrors has none: THIS COMMENT IS THE DEFINITION, its oracle is
 * float64 numpy.  Inputs: bank [N][D] f32 (the bank of w2v2_score_pairs), cohort [M][D] f32, pairs [P][2] int32 (column 0
 * the enrolment side e, column 1 the test side t), the evaluator's mean / std and length_norm.
 *   1. transform   u = (x - mean) / (std + 1e-12) when centring is on, then u / max(||u||, 1e-12) with length_norm: the
 *                  transform of w2v2_score_pairs, for bank rows and cohort rows alike.
 *   2. cosines     S[r][m] = u_r . c_m / (max(||u_r||, 1e-8) * max(||c_m||, 1e-8)): w2v2_gemm on f32 operands with
 *                  W2V2_EPI_SCALE_RC, row_scale / col_scale = the inv_norm of w2v2_rows_transform.  S is never held
 *                  whole: the host loops over blocks of bank rows and one caller-owned [rows_per_block][ldS] buffer.
 *   3. statistics  mu[r] = mean of the K largest values of S[r][:], sd[r] = their unbiased std (ddof = 1), 2 <= K <= M.
 *                  The top K is a multiset: with t the K-th largest value and g = #{v > t} the sum is
 *                  sum_{v > t} v + (K - g) t, so ties at t do not matter.  -0.0 equals +0.0.  A NaN anywhere in the row
 *                  gives mu = sd = NaN for that row only.
 *   4. score       z_e = (c - mu[e]) / (sd[e] + 1e-12) with c the raw cosine of the trial, z_t likewise with t;
 *                  mode 0 ("z") -> z_e, 1 ("t") -> z_t, 2 ("s") -> (z_e + z_t) / 2.  NOT mapped through (x + 1) / 2 and
 *                  not clipped (it is unbounded, and clipping is not monotone).  An index outside [0, N) gives NaN for
 *                  that trial only.
 * Conventions of the trial scoring above: 16-byte vectors, D % 4 == 0, ld % 4 == 0, 64-bit row offsets, no atomics on
 * global memory, no workgroup waits on another, fixed-order folds (equal inputs give equal bits), nothing allocated,
 * all work on `stream`.
 *
 * Step 1 for `rows` rows of x [rows][ld]: out [rows][ld_out] = the transformed rows, inv_norm [rows] = 1 / max(||u||, 1e-8)
 * of what was stored (the squares of a row are summed in double).  One pass over HBM (with length_norm a row is read a
 * second time out of the cache).  mean / std: both NULL or both set, [D], 16-byte aligned.  out may be NULL only when
 * neither centring nor length norm is asked for: only inv_norm is written and the product reads x itself.  out != x. */
int w2v2_rows_transform(const float* x, int64_t ld, int rows, int D, const float* mean, const float* std, int length_norm,
                        float* out, int64_t ld_out, float* inv_norm, void* stream);
/* Step 3 for the R rows of S [R][ldS] (ldS >= M, ldS % 4 == 0, 16-byte aligned; the columns behind M are never read).
 * One workgroup per row: an exact radix select of the K-th largest value over the order-preserving u32 image of the
 * values (four 8-bit histogram passes in LDS, most significant byte first), then the tie-aware sum and the centred second
 * moment about that mean, both in double, folded in a fixed order.  A row of at most w2v2_topk_stats_lds_keys() values is
 * staged in LDS; a longer one is re-read (from L2) in every pass; both routes give the same bits.  2 <= K <= M < 2^24,
 * anything else is an argument error. */
int w2v2_topk_stats_lds_keys(void);
int w2v2_topk_stats(const float* S, int64_t ldS, int R, int M, int K, float* mu, float* sd, void* stream);
/* Step 4: cos [P] as w2v2_score_pairs leaves it, pairs [P][2], mu / sd [N] of step 3 -> score_out [P].  One trial per
 * thread, in double, rounded once.  sd = 0 gives what the formula gives (a division by 1e-12), never a fault. */
int w2v2_score_pairs_norm(const float* cos, const int32_t* pairs, int P, const float* mu, const float* sd, int N, int mode,
                          float* score_out, void* stream);
/* The cohort builder: out [S][ld_out] = the mean of the bank rows of each of S segments (speakers).  order [N] int32 lists
 * the rows of bank [N][ld] grouped by segment, offsets [S + 1] int32 (offsets[0] = 0, offsets[S] = N) cuts it.  One
 * workgroup per segment and 128-dimension strip; row lane y of eight folds rows order[begin + y], order[begin + y + 8], ...
 * in that sequence in double, the lanes are folded in lane order.  An empty segment is the host's argument error; on the
 * device an empty or out-of-range segment, or a row number outside [0, N), is not dereferenced: that mean is NaN. */
int w2v2_segment_mean(const float* bank, int64_t ld, int N, int D, const int32_t* order, const int32_t* offsets, int S,
                      float* out, int64_t ld_out, void* stream);

/* ---------------------------------------------------------------------------------- scoring back-ends (backend.hip)
 * LDA and PLDA trial scoring beside the cosine back-end (ref: config/evaluator/{lda,plda}.yaml, src/evaluation/speaker/
 * lda.py and plda.py).  The reference's two classes cannot run as shipped (a constructor keyword its base class lacks, a
 * PCA hard-coded to 200 components, a PLDA library that is not installable, `10 ** llr` pushed through (s + 1) / 2), so
 * THIS COMMENT IS THE DEFINITION and its oracle is float64 numpy.  Kept from the reference: the constructor keywords and
 * the chain projection -> centring -> length norm -> score.  Inputs: a training bank X [N][D] f32 on the device, one
 * speaker label per row (host; mapped to 0 .. C-1 in sorted order, as the cohort builder does), an evaluation bank and
 * an int32 trial table as for w2v2_score_pairs.
 *   1. class statistics.  Counts n_c; class means m_c (w2v2_segment_mean); global mean mu0 (w2v2_embed_stats);
 *        S_w = sum_r (x_r - m_c(r)) (x_r - m_c(r))^T,   S_b = sum_c n_c (m_c - mu0) (m_c - mu0)^T,   S_t = S_w + S_b.
 *      A scatter matrix is formed block by block over at most rows_per_block rows: w2v2_rows_center writes the f32 block
 *      a_r = w_r (x_r - mean row), w2v2_gemm on f32 operands forms A^T A [D][D] in f32, w2v2_scatter_fold adds it into a
 *      [D][D] float64 accumulator (one writer per element, blocks in ascending order); the host symmetrises
 *      (S + S^T) / 2 in float64.  S_b runs over the C class-mean rows with w_c = sqrt(n_c) and mu0 subtracted.
 *   2. projection to R dimensions, y = P (x - mu0), P [R][D] solved on the host in float64 (symmetric eigen-solves).
 *      "pca": the top-R eigenpairs (lambda, v) of S_t / (N - 1), rows of P = v / sqrt(lambda) (whitening PCA: the
 *      projected training covariance is the identity); R <= min(D, N - 1).  "lda": whiten S_w / (N - C), then the top-R
 *      eigenvectors of the whitened S_b / (C - 1); R <= min(D, C - 1); the projected S_w / (N - C) is the identity.  A
 *      kept eigenvalue <= 1e-10 lambda_max is an error (a singular covariance).  The bank is projected by w2v2_gemm
 *      (f32) with a bias epilogue, b = -P mu0, into an [N][R4] bank, R4 = R rounded up to 4, pad columns zero.
 *      Eigenvector signs are left as the solver gives them: every score below is invariant to them.
 *   3. latent normalisation.  mean / std over the projected TRAINING rows (w2v2_embed_stats), then
 *      (y - mean) / (std + 1e-12) and F.normalize: the transform of w2v2_score_pairs / w2v2_rows_transform.  The LDA
 *      back-end stops here and scores with the cosine (w2v2_score_pairs on the projected bank, (s + 1) / 2 clipped).
 *   4. PLDA, the two-covariance model z = mu + y_c + e in the normalised latent space, y_c ~ N(0, B), e ~ N(0, W), mu
 *      fixed at the mean of the normalised training rows.  Statistics of step 1 over the normalised training rows
 *      Z [N][R]: n_c, m_c, S_w.  W_0 = S_w / N, B_0 = (1 / C) sum_c (m_c - mu)(m_c - mu)^T; max_iterations EM steps on
 *      the host in float64:
 *        E   Phi_c = (B^-1 + n_c W^-1)^-1,   yhat_c = Phi_c n_c W^-1 (m_c - mu)
 *        M   B = (1 / C) sum_c (Phi_c + yhat_c yhat_c^T)
 *            W = (1 / N) [ S_w + sum_c n_c ((m_c - mu - yhat_c)(m_c - mu - yhat_c)^T + Phi_c) ].
 *      Then A with A W A^T = I and A B A^T = diag(psi), psi descending; the first Q rows are kept and
 *      u = A (z - mu) is one more f32 GEMM with bias into an [N][Q4] bank.  The score of a trial (e, t):
 *        llr = k + sum_d p_d u_e,d u_t,d - sum_d q_d (u_e,d^2 + u_t,d^2)
 *        p_d = psi_d / (2 psi_d + 1),  q_d = psi_d^2 / (2 (psi_d + 1)(2 psi_d + 1)),
 *        k = sum_d [ log(psi_d + 1) - log(2 psi_d + 1) / 2 ],
 *      the exact log-ratio of the same-speaker joint Gaussian to the product of the marginals.  It is unbounded and
 *      goes to the metrics as it is: NOT through (s + 1) / 2 and not clipped.
 * Conventions of the trial scoring above: f32 banks, D % 4 == 0, ld % 4 == 0, 16-byte vectors, 64-bit row offsets, no
 * atomics on global memory, no workgroup waits on another, fixed-order folds (equal inputs give equal bits), nothing
 * allocated, all work on `stream`.
 *
 * out[r][:] = w_r * (x[r][:] - means[seg_id[r]][:]) for `rows` rows: one f32 subtraction and one f32 multiplication per
 * element, never contracted.  seg_id int32 [rows] or NULL (every row takes means[0]); means [S][ld_means]; row_weight f32
 * [rows] or NULL (w = 1).  A seg_id outside [0, S) is not dereferenced: that row of out is NaN.  out != x. */
int w2v2_rows_center(const float* x, int64_t ld, int rows, int D, const int32_t* seg_id /*int32 [rows] or NULL*/,
                     const float* means, int64_t ld_means, int S, const float* row_weight /*f32 [rows] or NULL*/, float* out,
                     int64_t ld_out, void* stream);
/* acc [D][D] f64 (row stride D, 16-byte aligned) = (first ? 0 : acc) + block [D][ldb] f32.  With first != 0 acc is not
 * read.  One writer per element; the sum over blocks takes the order of the calls. */
int w2v2_scatter_fold(const float* block /*f32 [D][ldb]*/, int64_t ldb, double* acc /*f64 [D][D]*/, int D, int first,
                      void* stream);
/* The llr of step 4 for P trials over the diagonalised bank u [N][ld] with Q columns (Q % 4 == 0: pad columns carry
 * p = q = 0); p, q f64 [Q] on the device, 16-byte aligned; k by value.  One trial per wavefront, one pass over the two
 * rows; every product is formed and summed in double, the lanes fold in a fixed order, one rounding to f32.  An index
 * outside [0, N) is not dereferenced: that trial is NaN. */
int w2v2_plda_score_pairs(const float* u, int64_t ld, int N, int Q, const int32_t* pairs /*int32 [P][2]*/, int P,
                          const double* p, const double* q, double k, float* llr_out /*[P]*/, void* stream);

/* ---------------------------------------------------------------------------------- trial metrics (metrics.hip)
 * What follows the scores: ROC / EER / minDCF of a trial list without the P scores leaving the device.  No kernel waits
 * on another workgroup (no look-back, no flag, no cooperative launch): every order between workgroups is a launch
 * boundary.  No atomics on global memory, integer counters only in LDS; results are bitwise reproducible.  Nothing is
 * allocated; all work goes on `stream`; workspaces are caller-owned and 16-byte aligned.
 *
 * Stable ascending argsort of keys [P] f32, 1 <= P < 2^31: order_out [P] int32 = np.argsort(keys, kind="stable") exactly
 * (-0.0 and +0.0 are equal and tie by index; every NaN, of either sign bit, sorts behind +inf, NaNs in index order);
 * keys_out [P] (may be NULL) = keys[order], the keys' own bits.  The order eval_metrics.py takes with two host argsorts
 * (ref: src/eval_metrics.py:54-79 through sklearn's roc_curve, and :90-206).  An LSD radix sort of the order-preserving
 * u32 image of the keys, 8 bits a pass: per pass a histogram per tile of w2v2_sort_tile() keys, a scan of the digit x tile
 * table and a stable scatter (rank in a tile by wave ballots and a fixed wave-order prefix).  workspace: at least
 * w2v2_sort_f32_index_workspace_bytes(P) bytes (-1: P out of range). */
int w2v2_sort_tile(void);
int64_t w2v2_sort_f32_index_workspace_bytes(int64_t P);
int w2v2_sort_f32_index(const float* keys, int64_t P, int32_t* order_out, float* keys_out, void* workspace, void* stream);
/* EER and minDCF of scores [P] f32 (as w2v2_score_pairs / w2v2_score_frame_sets leave them) with labels [P] uint8 (0 / 1),
 * both on the device (ref: src/eval_metrics.py:54-79 calculate_eer, :90-206 calculate_mdc and _compute_error_rates) ->
 * out [8] f64 on the device: eer, eer_threshold, mdc, mdc_threshold, n_pos, n_neg, n_nan, n_thresholds.
 *   The stable sort above, then integer-exact steps: cumulative positives over the order, group ends (a position whose
 * key differs from the next one's), the ROC points = the group ends in DESCENDING score order behind the origin
 * (0, 0, +inf), kept as sklearn's drop_intermediate keeps them (origin, first and last point; between them where the
 * second difference of fp or tp is non-zero; n_thresholds counts them).  EER: `1 - fp/N - tp/Pn <= 0` is tested as
 * fp*Pn + tp*N >= N*Pn in int64; hi = first kept point that passes, lo = last kept point that does not (two index
 * reductions); fp_lo == fp_hi: eer = fp_hi/N, threshold = thr_hi; otherwise the crossing of the segment with y = 1 - x and
 * the threshold interpolated along it; lo = origin: threshold +inf.  minDCF: c_det = c_miss*fnr*p_target +
 * c_fa*fpr*(1 - p_target) at EVERY position of the stable order (the minimum may fall inside a tie group), lowest index
 * among equal minima, evaluated in f64 without contraction so that it rounds as numpy does; mdc = min / min(c_miss*p_target,
 * c_fa*(1 - p_target)), mdc_threshold = the score there.
 *   n_nan = NaN scores; when it is non-zero, or when one class is absent, the other outputs are unspecified (never a
 * fault).  c_miss < 1, c_fa < 1 or p_target outside [0, 1] is an argument error, as in calculate_mdc.  workspace: at least
 * w2v2_trial_metrics_workspace_bytes(P) bytes (-1: P out of range). */
int64_t w2v2_trial_metrics_workspace_bytes(int64_t P);
int w2v2_trial_metrics(const float* scores, const uint8_t* labels, int64_t P, double c_miss, double c_fa, double p_target,
                       double* out, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------- score calibration (calibration.hip)
 * What turns trial scores into log-likelihood ratios, and what says how good they are as such: a prior-weighted logistic
 * regression of K systems' scores (K = 1: calibration; K > 1: linear fusion), its affine map applied on the device, and
 * Cllr / actDCF of the result.  The reference project has no calibration: THIS BLOCK IS THE DEFINITION.  Conventions of
 * the trial metrics above: no kernel waits on another workgroup, no atomics on global memory, per-workgroup partials in a
 * caller-owned 16-byte aligned workspace folded in ascending order by one workgroup, nothing allocated, all work on
 * `stream`.  Every sum and every transcendental is f64, no product is contracted into an fma, every fold has a fixed
 * order: equal inputs give equal bits.
 *
 * Inputs: scores S [K][P] f32 with row stride ld >= P (the pad behind a row is never read), 1 <= K <=
 * W2V2_CALIB_MAX_SYSTEMS, 1 <= P < 2^31; labels [P] uint8 (0 / 1); c_miss >= 1, c_fa >= 1, 0 < p_target < 1; ridge >= 0.
 *   pi = p_target c_miss / (p_target c_miss + (1 - p_target) c_fa), tau = log(pi / (1 - pi)), theta = -tau.
 * 1. Moments, two passes: m_k = sum_i s_ki / P; sd_k = sqrt(sum_i (s_ki - m_k)^2 / (P - 1)); r_k = 1 / sd_k;
 *    x_i = (1, (s_1i - m_1) r_1, ...); N_tar, N_non, n_nan (trials with a NaN in any system).
 * 2. At w in R^(K+1): l_i = w_0 + sum_k w_k x_ik (k ascending), z_i = l_i + tau, c_i = pi / N_tar (target) or
 *    (1 - pi) / N_non;  e = exp(-|z|), sigma(|z|) = 1 / (1 + e), sigma(-|z|) = e / (1 + e), softplus(a) = max(a, 0) +
 *    log1p(e);  J = sum c_i softplus(-z_i | target, z_i | non-target) + ridge / 2 sum_{k>=1} w_k^2;
 *    g = sum c_i (sigma(z_i) - y_i) x_i (a target's sigma - 1 is -sigma(-z), never a difference) + ridge w_k;
 *    H = sum c_i sigma(z_i) sigma(-z_i) x_i x_i^T + ridge on the diagonal behind element 0.
 * 3. Newton with step halving from w = 0 (or w_start): a trial point whose J exceeds the accepted J is rejected and the
 *    step along the kept direction halved; an accepted point gives d = H^-1 g by Cholesky and the decrement g.d / 2; the
 *    fit has converged when that is < 1e-12 -- unless ridge = 0 and J < min(pi / N_tar, (1 - pi) / N_non) ln 2 there: a
 *    trial on the wrong side of its threshold costs at least c_i ln 2, so such a J proves the set separable, J has no
 *    minimum (it only falls towards 0, by about e per round) and the fit keeps running -- else the next trial point is
 *    w - d.  status: 0 running (also: not converged
 *    after max_iter rounds), 1 converged, 2 H not positive definite / a non-finite sum / n_nan > 0 / sd_k = 0 or not
 *    finite / a class absent, 3 step below 2^-20.  The whole fit is enqueued by one call: two moment passes, then
 *    max_iter rounds of one tiled statistics launch and one single-workgroup fold + solve launch.  Once the status is
 *    non-zero the statistics launches return at once and the solve launches change nothing: the host never waits.
 * 4. a_k = w_k r_k, a_0 = w_0 - sum_k a_k m_k (k ascending): llr_i = a_0 + sum_k a_k s_ki.
 * The record, f64 [w2v2_calib_record_doubles()] on the device, written whole by every fit (N = K + 1, M =
 * W2V2_CALIB_MAX_SYSTEMS): [0] status, [1] rounds used, [2] K, [3] accepted J, [4] step, [5] last decrement, [6] N_tar,
 * [7] N_non, [8] n_nan, [9] J of the last trial point, [16 ..] accepted w [M + 1], then direction d [M + 1], trial w
 * [M + 1], m [M], sd [M], r [M], a [M + 1], g [M + 1] and H [M + 1][M + 1] of the accepted point.
 * w_start: HOST pointer to K + 1 doubles or NULL (w = 0); with max_iter = 1 the record then holds J, g and H at w_start.
 * workspace: at least w2v2_calib_workspace_bytes(P) bytes (-1: P out of range), one row per tile of w2v2_calib_tile()
 * trials; it serves w2v2_llr_metrics as well. */
#define W2V2_CALIB_MAX_SYSTEMS 8
int w2v2_calib_tile(void);
int w2v2_calib_record_doubles(void);
int64_t w2v2_calib_workspace_bytes(int64_t P);
int w2v2_calib_fit(const float* scores, int64_t ld, int K, const uint8_t* labels, int64_t P, double c_miss, double c_fa,
                   double p_target, double ridge, int max_iter, const double* w_start, double* record, void* workspace,
                   void* stream);
/* 5. llr_out[i] = f32(a[0] + sum_k a[k + 1] (double)s_ki), k ascending, every product and sum in double, one rounding.
 * a: K + 1 doubles ON THE DEVICE (a fit's record + 16 + 3 (M + 1) + 3 M doubles: fit -> apply needs no host round trip).
 * A NaN score gives a NaN llr.  llr_out may not overlap scores. */
int w2v2_calib_apply(const float* scores, int64_t ld, int K, int64_t P, const double* a, float* llr_out, void* stream);
/* 6. llr [P] f32 and labels [P] uint8 on the device -> out [8] f64 on the device: cllr, cllr_tar, cllr_non, act_dcf,
 * act_p_miss, act_p_fa, n_pos, n_nan.  cllr_tar = mean over targets of log2(1 + e^-llr), cllr_non = mean over non-targets
 * of log2(1 + e^llr) (softplus in nats as in step 2, the mean divided by ln 2), cllr their mean.  act_p_miss = #(target,
 * llr < theta) / N_tar, act_p_fa = #(non-target, llr >= theta) / N_non: integer-exact counts, the comparison in double
 * against theta = -log(pi / (1 - pi)) as the host computes it; act_dcf = (c_miss p_miss p_target + c_fa p_fa
 * (1 - p_target)) / min(c_miss p_target, c_fa (1 - p_target)), calculate_mdc's expression, order and normaliser (ref:
 * src/eval_metrics.py:90-206).  0 <= p_target <= 1 here.  NaN llrs are counted in n_nan and make the cllr of their class
 * (and cllr) NaN: with both classes present, cllr is NaN exactly when n_nan > 0.  With a class absent the outputs that
 * divide by its count are NaN or inf (never a fault). */
int w2v2_llr_metrics(const float* llr, const uint8_t* labels, int64_t P, double c_miss, double c_fa, double p_target,
                     double* out, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------ layer mix (layer_mix.hip)
 * What connects the wav2vec2 encoder to the ECAPA-TDNN back-end: a learned softmax-weighted sum of ALL J = L + 1 hidden
 * states (prologue output, then layer 1 .. L), instance-normalised over time, written into the back-end's feature buffer.
 * The reference project has no such model (its wav2vec_xvector.py points the same way: a pre-trained front-end into a
 * TDNN back-end, frozen for the first steps); the recipe is the one published with UniSpeech's speaker-verification
 * downstream, restated from memory: THIS BLOCK IS THE DEFINITION.  No atomics, fixed summation orders: equal inputs
 * give equal bits.
 *
 * Inputs: xs = DEVICE table of J base pointers (1 <= J <= W2V2_LAYER_MIX_MAX_STATES) to hidden states x_j [B * T][H]
 * (contiguous rows, dtype_x f32 / bf16 / f16, 16-byte aligned); logits a [J] f32; lens = int32 [B] frame counts n_b on the
 * device (clamped to 0 .. T) or NULL (n_b = T).  H must be a multiple of 8 (16-byte vector accesses of 8 channels).
 * Forward:
 *   1. w = softmax(a) in f32, max-subtracted (written to w_out [J] when that is not NULL).
 *   2. m = sum_j w_j x_j: f32, ascending j, one fused multiply-add per term.
 *   3. mu[b,c] = (1 / n_b) sum_{t < n_b} m.
 *   4. var[b,c] = (1 / n_b) sum_{t < n_b} (m - mu)^2 -- biased, centred, never E[m^2] - mu^2.
 *   5. r = 1 / sqrt(var + 1e-5), saved as f32 rstd [B][H].
 *   6. y[b,t,c] = (m - mu) r for t < n_b and 0 for t >= n_b; y is f32 or bf16 (one rounding) with row stride ldy >= H
 *      (a multiple of 8); columns >= H of a row are not touched.
 *   instance_norm = 0: y = m (0 past n_b), no statistics, rstd untouched.
 * The sums over t depend on (n_b, c) only: a row with a length equals, bit for bit, the utterance alone in a (1, n_b)
 * launch.  m is staged in LDS up to W2V2_LAYER_MIX_LDS_FRAMES frames; longer inputs need `stage`, f32 [B * T][H] (NULL
 * otherwise).  Every hidden state is read once either way.
 * Backward (training, no lengths form): g = dL/dy and the stored y (dtype_g f32 / bf16, row strides ldg / ldy), rstd.
 *   s1[b,c] = mean_t g;  s2[b,c] = mean_t (g y);  dm = r ((g - s1) - y s2), f32 [B * T][H]  (instance_norm = 0: dm = g);
 *   the two means, dm and the products dm x_j are carried in f64 (rstd reaches 316 where a channel hardly moves, and a mean
 *   rounded to f32 then leaves 316 ulp per frame in every d_j); only the stored dm is rounded, once, to f32;
 *   d_j = sum_{b,t,c} dm x_j: per thread, per workgroup (one f64 each in the 16-byte aligned workspace of
 *   w2v2_layer_mix_workspace_floats floats, -1 for bad arguments), then folded in a fixed order by a second launch;
 *   grad_logits[j] += w_j (d_j - sum_k w_k d_k)  (ADDED: the arena's zero_grad clears it).
 * w2v2_scale_add: G = (overwrite ? 0 : G) + (sum_{j = lo .. hi} w_j) dm over n elements (a multiple of 8): the weights
 * summed in f32 in ascending j, one fused multiply-add, one rounding to G's dtype (f32 / bf16 / f16); dm is f32 or bf16;
 * w stays on the device.  It injects the mix's gradient into the encoder's running activation gradient. */
#define W2V2_LAYER_MIX_MAX_STATES 32
#define W2V2_LAYER_MIX_LDS_FRAMES 512
int w2v2_layer_mix_fwd(const void* const* xs, const float* logits, int J, const int* lens, void* y, int64_t ldy, float* rstd,
                       float* w_out, float* stage, int B, int T, int H, int instance_norm, int dtype_x, int dtype_y,
                       void* stream);
int64_t w2v2_layer_mix_workspace_floats(int B, int T, int H, int J);
int w2v2_layer_mix_bwd(const void* const* xs, const float* logits, int J, const void* g, int64_t ldg, const void* y,
                       int64_t ldy, const float* rstd, float* dm, float* grad_logits, float* workspace, int B, int T, int H,
                       int instance_norm, int dtype_x, int dtype_g, void* stream);
int w2v2_scale_add(void* G, const void* dm, const float* w, int lo, int hi, int overwrite, int64_t n, int dtype_g,
                   int dtype_dm, void* stream);

/* ------------------------------------------------------------------------------------ optimiser
 * torch.optim.Adam (ref: config/optim/algo/adam.yaml, src/main.py:323-335) over one flat f32
 * parameter arena; also refreshes the 16-bit copy (pb_dtype = W2V2_BF16 / W2V2_F16) the GEMMs read
 * (pb may be NULL).  grad_scale folds the 1/world_size of the data-parallel average.
 * scaler_state (may be NULL): the 4-float device record of w2v2_grad_scaler_*: gradients are divided by
 * state[0] and the whole step is skipped when state[1] != 0. */
/* skip_slot (0 = off, 4 or 5): torch's GradScaler does not call optimizer.step() on an overflow, so Adam's step count
 * must not advance on skipped steps.  With skip_slot set the kernel rebuilds both bias corrections from
 * t = step - scaler_state[skip_slot] (the host's `step` counts every call; the 8-float record counts the skipped ones
 * per parameter range: [4] head, [5] body -- see w2v2_grad_scaler_update) and ignores bias_corr1 / bias_corr2. */
int w2v2_adam_step(float* p, const float* g, float* m, float* v, void* pb, int pb_dtype, int64_t n, float lr,
                   float beta1, float beta2, float eps, float bias_corr1, float bias_corr2,
                   float grad_scale, const float* scaler_state, int step, int skip_slot, void* stream);

/* General optimiser step: torch.optim.Adam with L2 weight decay (grad += weight_decay * p, not AdamW) or
 * torch.optim.SGD (ref: config/optim/algo/adam.yaml, config/optim/algo/sgd.yaml: momentum 0.9, dampening 0, Nesterov,
 * weight decay; built at src/main.py:323-335), with the gradient-norm clipping of PL's `trainer.gradient_clip_val`
 * (torch.nn.utils.clip_grad_norm_) folded in.  Per element: gr = g * grad_scale / scaler_state[0] * norm_state[1]
 * + weight_decay * p, i.e. unscale, then clip, then decay.
 *   algo = W2V2_OPTIM_ADAM: the update of w2v2_adam_step on gr.  With weight_decay == 0 and norm_state == NULL the call
 *     IS w2v2_adam_step (forwarded: same kernel, same bits).
 *   algo = W2V2_OPTIM_SGD: buf = gr on the first step of the range that was not skipped, else
 *     buf = momentum * buf + (1 - dampening) * gr;  p -= lr * (nesterov ? gr + momentum * buf : buf).  The buffer lives
 *     in `m`; `v`, beta1, beta2, eps and the bias corrections are ignored (v may be NULL; m too when momentum == 0).
 *     "First" is t = step - scaler_state[skip_slot] <= 1 (t = step without skip_slot), the count Adam's bias correction uses.
 * norm_state (may be NULL): the {total_norm, clip_coef} record of w2v2_grad_norm; a zero coefficient (non-finite norm)
 * skips the whole step, like scaler_state[1] != 0.  The 16-bit copy pb is refreshed as in w2v2_adam_step. */
#define W2V2_OPTIM_ADAM 0
#define W2V2_OPTIM_SGD 1
int w2v2_optim_step(int algo, float* p, const float* g, float* m, float* v, void* pb, int pb_dtype, int64_t n, float lr,
                    float beta1, float beta2, float eps, float bias_corr1, float bias_corr2, float grad_scale,
                    float weight_decay, float momentum, float dampening, int nesterov, const float* norm_state,
                    const float* scaler_state, int step, int skip_slot, void* stream);

/* Global L2 norm of g[0..n) and the clip coefficient (torch.nn.utils.clip_grad_norm_, which PL calls after
 * GradScaler.unscale_ for `trainer.gradient_clip_val`; ref: config/trainer/trainer.yaml).
 * Every element is first multiplied by grad_scale / scaler_state[0] (plain grad_scale when scaler_state is NULL), squares
 * are summed in double.  Two launches, no atomics: one partial per workgroup, reduced in a fixed order, then one workgroup
 * adds the partials in index order; the grid depends on n alone, so equal bytes give equal bits on every launch and rank.
 *   norm_state[0] = total_norm,  norm_state[1] = min(1, max_norm / (total_norm + 1e-6))   (1 when max_norm <= 0).
 * A non-finite norm gives norm_state[1] = 0 and, with a record, scaler_state[1] = 1 (found_inf): the pass has read the
 * whole slice, so it replaces w2v2_grad_scaler_check for that step.  partials: caller-owned, n_partials doubles,
 * at least w2v2_grad_norm_partials of n (never more than 1024). */
int w2v2_grad_norm_partials(int64_t n);
int w2v2_grad_norm(const float* g, int64_t n, float grad_scale, float* scaler_state, float max_norm, double* partials,
                   int n_partials, float* norm_state, void* stream);

/* Gradient accumulation over the micro-batches of one optimiser step: PL `trainer.accumulate_grad_batches` = N (ref:
 * config/trainer/trainer.yaml:33) makes N backward passes of loss / N add into .grad before optimizer.step().  Every
 * backward here WRITES its gradient arena, so the window's sum is kept in a second f32 arena of the same layout:
 *   first != 0:  acc[i] = g[i]            (acc is never read: a new window needs no zeroing pass)
 *   first == 0:  acc[i] = acc[i] + g[i]   (plain f32 add, the bits of torch's acc + g)
 * The sum stays unscaled: 1 / (world * N) belongs in grad_scale of w2v2_optim_step / w2v2_adam_step / w2v2_grad_norm.
 * acc and g 16-byte aligned (arena slices are 64-element aligned), n >= 0 (n == 0: no launch). */
int w2v2_grad_accumulate(float* acc, const float* g, int64_t n, int first, void* stream);

/* Dynamic loss scaling for fp16 activations = torch.cuda.amp.GradScaler, which PL `precision: 16` of the
 * reference's runs installs (ref: config/experiment/speaker_wav2vec2_aam.yaml:17).
 * state (device, 4 floats, or 8 with per-range skip counts) = {scale, found_inf, growth_tracker, skipped_steps
 * [, skipped_head, skipped_body, 0, 0]}; the heads multiply the loss
 * gradient by state[0] (w2v2_aam_softmax_fwd_bwd / w2v2_bce_head_fwd_bwd `loss_scale`), so every gradient of the
 * step carries it.  check: state[1] = 1 if any of g[0..n) is non-finite.  update (after the optimiser step):
 * found_inf ? scale *= backoff : (every growth_interval clean steps scale *= growth); clears found_inf.
 * No host synchronisation anywhere. */
/* lo[off_i .. off_i + n_i) = fp16(p[..] - fp16(p[..])) for every (off_i, n_i) of `table` ([n_ranges][2] int64, device):
 * the residual plane of the two-term weights above (p = f32 master arena, lo = a 16-bit arena of the same layout). */
int w2v2_weight_residual(const float* p, void* lo, const int64_t* table, int n_ranges, int dtype, void* stream);
int w2v2_grad_scaler_check(const float* g, int64_t n, float* state, void* stream);
/* skipped_ranges: bit 0 / bit 1 = on an overflow also count the skipped step in state[4] / state[5] (records of 8
 * floats; pass 0 for the plain 4-float record). */
int w2v2_grad_scaler_update(float* state, float growth, float backoff, int growth_interval, int skipped_ranges,
                            void* stream);

/* ------------------------------------------------------------------------------------ collective
 * ref: config/trainer/trainer.yaml:6-12 (PL `accelerator: ddp`, one process per GPU): the SUM all-reduce of the gradient
 * buckets is the only collective of a data-parallel step.  The repo's default binding issues it through
 * torch.distributed ("nccl" == RCCL); these three calls run the same collective through the C ABI alone, on RCCL over
 * xGMI (librccl.so resolved with dlopen at the first call -- no link-time dependency; W2V2_RCCL_LIB overrides the path).
 *   rank 0: w2v2_comm_unique_id(id) -> ship the 128 bytes to every rank out of band (file, socket, launcher env)
 *   every rank: w2v2_comm_init(&c, id, rank, world, device)             (collective: all ranks must call it)
 *   per bucket: w2v2_allreduce_async(c, grad + off, n, comm_stream)     (in place, f32, enqueued on the given stream;
 *               order the stream against the backward with events, like trainer.BucketAllReducer does)
 *   at start-up / after loading a checkpoint on one rank: w2v2_broadcast_async(c, buf, nbytes, root, stream) of the
 *               parameter arena, the optimiser moments and the loss-scale record (in place, any dtype: bytes) -- what
 *               PL's DDP wrapper does implicitly when it wraps the module (identical replicas)
 *   w2v2_comm_destroy(c)
 * Multi-rank operation of these entry points is covered by construction + a world-size-1 communicator on the 1-GPU test
 * boxes; the first check on an N-GPU node is tools/scale_sweep.sh (2 ranks against torch.distributed, bitwise). */
typedef struct w2v2_comm w2v2_comm;
int w2v2_comm_unique_id(void* id_host_128);
int w2v2_comm_init(w2v2_comm** comm, const void* id_host_128, int rank, int world, int device);
/* Loop-back communicator (tests / single-GPU rehearsals; no RCCL involved): stands for rank 0 of a `world`-rank job whose
 * peers hold bit-identical buffers -- w2v2_allreduce_async multiplies the buffer by `world` on the stream (the SUM of
 * `world` equal contributions), w2v2_broadcast_async leaves it as it is.  It lets the world > 1 code path of a caller
 * (bucket order, side stream, 1/world scaling, start-up broadcast) run on a box with one GPU, where RCCL refuses two
 * ranks per device. */
int w2v2_comm_init_loopback(w2v2_comm** comm, int world, int device);
int w2v2_allreduce_async(w2v2_comm* comm, float* buf, int64_t n, void* stream);
int w2v2_broadcast_async(w2v2_comm* comm, void* buf, int64_t nbytes, int root, void* stream);
int w2v2_comm_destroy(w2v2_comm* comm);
/* Tools only (tools/overlap_rehearsal.py): a stand-in for the RCCL channels of one bucket's all-reduce on a 1-GPU box --
 * `channels` workgroups holding `lds_bytes` of LDS each stream the n floats of `buf` through themselves in place (values
 * unchanged), paced to `gbps` GB/s in total (0 = unpaced).  Measures what the collective's residency costs the compute
 * stream; moves nothing between GPUs. */
int w2v2_traffic_probe(float* buf, int64_t n, int channels, int lds_bytes, float gbps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
