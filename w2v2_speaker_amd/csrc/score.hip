// Trial scoring on the device (f32 banks, gfx950, wave64): the last arithmetic stage of the speaker path.
//   w2v2_embed_stats       per-dimension mean / unbiased std of an embedding bank (CosineDistanceEvaluator.fit_parameters)
//   w2v2_score_pairs       cosine score of a trial list over an [N, D] bank, optional z-score + length norm
//   w2v2_score_frame_sets  the non-pooled score: mean of all pairwise frame cosines of two frame sets
// Conventions of the f32 strip kernels: a thread reads one 16-byte vector of 4 features per step, every guard is per
// vector (D % 4 == 0, ld % 4 == 0), every row * ld is formed in 64 bits, no atomics and fixed-order folds (bitwise
// reproducible), nothing allocated here, everything on the caller's stream.  The NaN of a bad trial, the centring of one
// vector and the host's row-buffer check are those of every evaluation stage: trial_common.h.
#include "trial_common.h"

namespace {

// (cos + 1) / 2 clipped to [0, 1] (ref: speaker_recognition_evaluator.py:81); NaN stays NaN
__device__ __forceinline__ float score_of(double c) {
  const double s = (c + 1.0) * 0.5;
  return (float)(s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s));
}

// ------------------------------------------------------------------------------------------ embed_stats
// The scheme of conv0.hip / wav2spk.hip.  (1) partial: a workgroup takes ST_ROWS rows and a 128-dimension strip, holds its
// rows in registers, and writes per dimension the chunk mean and the CENTRED second moment sum (x - mean_chunk)^2, both
// summed in double and stored as doubles (strip_centred_moments: E[x^2] - mean^2 is never formed: a dimension with mean 1e3
// and std 1e-2 would lose ten digits, and a constant dimension would not come out with std exactly 0).  (2) one thread
// per dimension combines the chunks in double, in chunk order (Chan et al.: M2 += M2_j + delta^2 n n_j / (n + n_j)).
using StGeom = StripGeom<float>;
constexpr int ST_ROWS = 128, ST_RPT = ST_ROWS / StGeom::RL;

__global__ __launch_bounds__(256) void stats_partial_kernel(const float* __restrict__ bank, int64_t ld, int N, int D,
                                                            double* __restrict__ partial) {
  __shared__ double red[StGeom::RL][STRIP_CW];
  __shared__ float mu_s[STRIP_CW];
  const int blk = blockIdx.y;
  const int r0 = blk * ST_ROWS;
  const int n = min(ST_ROWS, N - r0);                       // >= 1: the grid has cdiv(N, ST_ROWS) chunks
  const int cg = blockIdx.x * STRIP_CW + threadIdx.x * 4;
  const int tid = threadIdx.y * StGeom::XL + threadIdx.x;
  double mean_d, m2;
  strip_centred_moments<ST_RPT>(bank + (int64_t)r0 * ld + cg, ld, n, cg < D, red, mu_s, mean_d, m2);
  const int cc = blockIdx.x * STRIP_CW + tid;
  if (tid < STRIP_CW && cc < D) {
    double* dst = partial + ((int64_t)blk * D + cc) * 2;
    dst[0] = mean_d;
    dst[1] = m2;
  }
}

// (count, mean, M2) of a run of rows joined with those of the rows behind it
__device__ __forceinline__ void chan_join(double& cnt, double& mean, double& m2, double nj, double mj, double qj) {
  const double delta = mj - mean, tot = cnt + nj, r = nj / tot;
  mean += delta * r;
  m2 += qj + delta * delta * cnt * r;
  cnt = tot;
}
// A workgroup folds SF_DIMS dimensions: the chunks are cut into SF_SEG runs of consecutive chunks, thread (seg, dim) joins
// the chunks of its run in chunk order, then the thread of run 0 joins the runs in run order -- the same tree for a given
// N in every launch (a single thread per dimension would walk 1135 dependent steps at 145,160 rows).
constexpr int SF_SEG = 16, SF_DIMS = 16;

__global__ __launch_bounds__(SF_SEG * SF_DIMS) void stats_fold_kernel(const double* __restrict__ partial, int N, int D,
                                                                      float* __restrict__ mean_out,
                                                                      float* __restrict__ std_out) {
  __shared__ double run_s[3][SF_SEG][SF_DIMS];
  const int cl = threadIdx.x % SF_DIMS, seg = threadIdx.x / SF_DIMS;
  const int c = blockIdx.x * SF_DIMS + cl;
  const int nb = (N + ST_ROWS - 1) / ST_ROWS, per = (nb + SF_SEG - 1) / SF_SEG;
  const int j0 = seg * per, j1 = min(nb, j0 + per);
  double mean = 0.0, m2 = 0.0, cnt = 0.0;
  if (c < D)
    for (int j = j0; j < j1; ++j) {
      const double* src = partial + ((int64_t)j * D + c) * 2;
      chan_join(cnt, mean, m2, (double)min(ST_ROWS, N - j * ST_ROWS), src[0], src[1]);
    }
  run_s[0][seg][cl] = cnt; run_s[1][seg][cl] = mean; run_s[2][seg][cl] = m2;
  __syncthreads();
  if (seg != 0 || c >= D) return;
  for (int s = 1; s < SF_SEG; ++s)
    if (run_s[0][s][cl] > 0.0) chan_join(cnt, mean, m2, run_s[0][s][cl], run_s[1][s][cl], run_s[2][s][cl]);   // (run 0 is never empty)
  mean_out[c] = (float)mean;
  std_out[c] = (float)sqrt(m2 / (double)(N - 1));           // unbiased, as torch.std_mean
}

// ------------------------------------------------------------------------------------------ score_pairs
// One trial per wavefront, four per workgroup, one pass over the two rows.  A lane folds its vectors in ascending order in
// f32, the 64 lane sums are folded in double (xor butterfly: the same tree in every run), and the few operations per trial
// behind them run in double and round once.
constexpr int SP_WAVES = 4;

template <bool CENTER>
__global__ __launch_bounds__(SP_WAVES * 64) void score_pairs_kernel(const float* __restrict__ bank, int64_t ld, int N, int D,
                                                                    const int* __restrict__ pairs, int P,
                                                                    const float* __restrict__ mean,
                                                                    const float* __restrict__ sd, int length_norm,
                                                                    float* __restrict__ cos_out,
                                                                    float* __restrict__ score_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = (int64_t)blockIdx.x * SP_WAVES + wave;
  if (p >= P) return;                                       // (a whole wave; the kernel has no barrier)
  const int i = pairs[2 * p], j = pairs[2 * p + 1];
  if (i < 0 || i >= N || j < 0 || j >= N) {                 // not dereferenced (kept local: trial_common.h says why)
    if (lane == 0) { cos_out[p] = qnan(); score_out[p] = qnan(); }
    return;
  }
  const float* __restrict__ ra = bank + (int64_t)i * ld;
  const float* __restrict__ rb = bank + (int64_t)j * ld;
  float ab = 0.f, aa = 0.f, bb = 0.f;
#pragma unroll 2
  for (int d = lane * 4; d < D; d += 256) {
    float4 a = ld4(ra + d), b = ld4(rb + d);
    if constexpr (CENTER) {
      const float4 m = ld4(mean + d), s = ld4(sd + d);
      a = centre4(a, m, s);
      b = centre4(b, m, s);
    }
    ab = fmaf(a.x, b.x, ab); ab = fmaf(a.y, b.y, ab); ab = fmaf(a.z, b.z, ab); ab = fmaf(a.w, b.w, ab);
    aa = fmaf(a.x, a.x, aa); aa = fmaf(a.y, a.y, aa); aa = fmaf(a.z, a.z, aa); aa = fmaf(a.w, a.w, aa);
    bb = fmaf(b.x, b.x, bb); bb = fmaf(b.y, b.y, bb); bb = fmaf(b.z, b.z, bb); bb = fmaf(b.w, b.w, bb);
  }
  double sab = wave_sum_d((double)ab), saa = wave_sum_d((double)aa), sbb = wave_sum_d((double)bb);
  if (lane != 0) return;
  if (length_norm) {                                        // F.normalize: x / max(||x||, 1e-12); the three sums rescale
    const double ia = 1.0 / fmax(sqrt(saa), 1e-12), ib = 1.0 / fmax(sqrt(sbb), 1e-12);
    sab *= ia * ib;
    saa *= ia * ia;
    sbb *= ib * ib;
  }
  // torch's cosine_similarity: each norm clamped on its own
  const double c = sab / (fmax(sqrt(saa), 1e-8) * fmax(sqrt(sbb), 1e-8));
  cos_out[p] = (float)c;
  score_out[p] = score_of(c);
}

// ------------------------------------------------------------------------------------------ score_frame_sets
// mean_{i,j} cos(l_i, r_j) = < mean_i l_i / max(||l_i||, 1e-8) , mean_j r_j / max(||r_j||, 1e-8) >: exact because torch
// clamps the two norms separately.  One workgroup per trial.  Pass 1: wave w takes positions w, w + 4, ... of each side and
// writes 1 / max(norm, 1e-8) of each row to LDS.  Pass 2, per strip of 256 features: every wave folds its rows (ascending
// position) scaled by those, the four partial sums go through LDS and wave 0 adds them in wave order and accumulates the
// strip's part of the dot product.  A row is read twice, the second time out of the cache.  Sums run in double.
constexpr int FS_WAVES = 4, FS_MAX_W = 256;

__global__ __launch_bounds__(FS_WAVES * 64) void score_frame_sets_kernel(const float* __restrict__ frames, int64_t ld,
                                                                         int64_t rows, int D, const int* __restrict__ sel,
                                                                         const int* __restrict__ counts, int W,
                                                                         float* __restrict__ cos_out,
                                                                         float* __restrict__ score_out) {
  __shared__ int sel_s[2][FS_MAX_W];
  __shared__ double inv_s[2][FS_MAX_W];
  __shared__ double part[FS_WAVES][2][4][64];
  __shared__ int bad_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = blockIdx.x;
  const int cnt[2] = {counts[2 * p], counts[2 * p + 1]};
  if (threadIdx.x == 0) bad_s = (cnt[0] <= 0 || cnt[1] <= 0 || cnt[0] > W || cnt[1] > W) ? 1 : 0;
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * W; e += FS_WAVES * 64) {
    const int side = e / W, pos = e - side * W;
    if (pos < cnt[side] && cnt[side] <= W) {
      const int r = sel[(p * 2 + side) * W + pos];
      sel_s[side][pos] = r;
      if (r < 0 || (int64_t)r >= rows) bad_s = 1;           // (every writer stores the same value)
    }
  }
  __syncthreads();
  if (bad_s) {                                              // the whole workgroup; no frame was read
    if (threadIdx.x == 0) { cos_out[p] = qnan(); score_out[p] = qnan(); }
    return;
  }
  for (int side = 0; side < 2; ++side)
    for (int pos = wave; pos < cnt[side]; pos += FS_WAVES) {
      const float* __restrict__ row = frames + (int64_t)sel_s[side][pos] * ld;
      double ss = 0.0;
      for (int d = lane * 4; d < D; d += 256) {
        const float4 v = ld4(row + d);
        ss = fma((double)v.x, (double)v.x, ss); ss = fma((double)v.y, (double)v.y, ss);
        ss = fma((double)v.z, (double)v.z, ss); ss = fma((double)v.w, (double)v.w, ss);
      }
      ss = wave_sum_d(ss);
      if (lane == 0) inv_s[side][pos] = 1.0 / fmax(sqrt(ss), 1e-8);
    }
  __syncthreads();
  double dot = 0.0;                                         // (wave 0)
  for (int d0 = 0; d0 < D; d0 += 256) {
    const int d = d0 + lane * 4;
    double acc[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    if (d < D) {
#pragma unroll
      for (int side = 0; side < 2; ++side)
        for (int pos = wave; pos < cnt[side]; pos += FS_WAVES) {
          const float4 v = ld4(frames + (int64_t)sel_s[side][pos] * ld + d);
          const double iv = inv_s[side][pos];
          acc[side][0] = fma((double)v.x, iv, acc[side][0]); acc[side][1] = fma((double)v.y, iv, acc[side][1]);
          acc[side][2] = fma((double)v.z, iv, acc[side][2]); acc[side][3] = fma((double)v.w, iv, acc[side][3]);
        }
    }
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
      for (int e = 0; e < 4; ++e) part[wave][side][e][lane] = acc[side][e];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double l = part[0][0][e][lane], r = part[0][1][e][lane];
#pragma unroll
        for (int w = 1; w < FS_WAVES; ++w) { l += part[w][0][e][lane]; r += part[w][1][e][lane]; }
        dot = fma(l, r, dot);
      }
    }
    __syncthreads();                                        // (part is rewritten by the next strip)
  }
  if (wave == 0) {
    dot = wave_sum_d(dot);
    if (lane == 0) {
      const double c = dot / ((double)cnt[0] * (double)cnt[1]);
      cos_out[p] = (float)c;
      score_out[p] = score_of(c);
    }
  }
}

}  // namespace

extern "C" int w2v2_embed_stats(const float* bank, int64_t ld, int N, int D, float* mean_out, float* std_out,
                                void* workspace, void* stream) {
  W2V2_REQUIRE(rows_ok(bank, ld, N, D) && mean_out && std_out && workspace && ((uintptr_t)workspace & 7) == 0,
               "embed_stats: bad arguments (D %% 4 == 0, ld >= D, ld %% 4 == 0, 16-byte aligned bank, 8-byte aligned workspace)");
  W2V2_REQUIRE(N >= 2, "embed_stats: the unbiased std needs N >= 2 rows (got %d)", N);
  const int nchunk = (int)cdiv(N, ST_ROWS);
  W2V2_REQUIRE(nchunk <= 65535, "embed_stats: N = %d is more than 65535 chunks of %d rows", N, ST_ROWS);
  hipLaunchKernelGGL(stats_partial_kernel, dim3((unsigned)cdiv(D, STRIP_CW), (unsigned)nchunk), dim3(StGeom::XL, StGeom::RL), 0,
                     as_stream(stream), bank, ld, N, D, (double*)workspace);
  W2V2_CHECK_LAUNCH("embed_stats(partial)");
  hipLaunchKernelGGL(stats_fold_kernel, dim3((unsigned)cdiv(D, SF_DIMS)), dim3(SF_SEG * SF_DIMS), 0, as_stream(stream),
                     (const double*)workspace, N, D, mean_out, std_out);
  W2V2_CHECK_LAUNCH("embed_stats(fold)");
  return 0;
}

extern "C" int w2v2_score_pairs(const float* bank, int64_t ld, int N, int D, const int32_t* pairs, int P, const float* mean,
                                const float* std_, int length_norm, float* cos_out, float* score_out, void* stream) {
  W2V2_REQUIRE(rows_ok(bank, ld, N, D) && pairs && P > 0 && cos_out && score_out,
               "score_pairs: bad arguments (D %% 4 == 0, ld >= D, ld %% 4 == 0, 16-byte aligned bank)");
  W2V2_REQUIRE((mean == nullptr) == (std_ == nullptr), "score_pairs: mean and std are both null or both set");
  W2V2_REQUIRE(!mean || ((((uintptr_t)mean) | ((uintptr_t)std_)) & 15) == 0, "score_pairs: mean / std must be 16-byte aligned");
  const dim3 grid((unsigned)cdiv(P, SP_WAVES)), block(SP_WAVES * 64);
  if (mean)
    hipLaunchKernelGGL(score_pairs_kernel<true>, grid, block, 0, as_stream(stream), bank, ld, N, D, pairs, P, mean, std_,
                       length_norm, cos_out, score_out);
  else
    hipLaunchKernelGGL(score_pairs_kernel<false>, grid, block, 0, as_stream(stream), bank, ld, N, D, pairs, P, mean, std_,
                       length_norm, cos_out, score_out);
  W2V2_CHECK_LAUNCH("score_pairs");
  return 0;
}

extern "C" int w2v2_score_frame_sets(const float* frames, int64_t ld, int64_t rows, int D, const int32_t* sel,
                                     const int32_t* counts, int W, int P, float* cos_out, float* score_out, void* stream) {
  W2V2_REQUIRE(rows_ok(frames, ld, rows, D) && sel && counts && P > 0 && cos_out && score_out,
               "score_frame_sets: bad arguments (D %% 4 == 0, ld >= D, ld %% 4 == 0, 16-byte aligned frames)");
  W2V2_REQUIRE(W >= 1 && W <= FS_MAX_W, "score_frame_sets: W = %d outside [1, %d]", W, FS_MAX_W);
  hipLaunchKernelGGL(score_frame_sets_kernel, dim3((unsigned)P), dim3(FS_WAVES * 64), 0, as_stream(stream), frames, ld, rows, D,
                     sel, counts, W, cos_out, score_out);
  W2V2_CHECK_LAUNCH("score_frame_sets");
  return 0;
}
