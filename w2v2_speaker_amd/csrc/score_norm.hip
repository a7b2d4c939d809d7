// Adaptive score normalisation on the device (f32, gfx950, wave64): the stage between score.hip and metrics.hip.
//   w2v2_rows_transform     the evaluator's transform of a bank or a cohort, and 1 / max(||u||, 1e-8) of every row
//   w2v2_topk_stats         mean and unbiased std of the K largest values of every row of S [R, M] (exact selection)
//   w2v2_score_pairs_norm   z / t / s normalisation of the raw cosines of a trial list
//   w2v2_segment_mean       per-speaker mean embeddings (the cohort builder)
// THE DEFINITION (include/w2v2_hip.h repeats it as the contract; nothing else defines this feature -- the project this
// one mirrors has no score normalisation, the oracle is float64 numpy):
//   1. transform   u = (x - mean) / (std + 1e-12) when centring is on, then u / max(||u||, 1e-12) with length_norm:
//                  the transform of w2v2_score_pairs, applied to bank rows and cohort rows alike.
//   2. cosines     S[r, m] = u_r . c_m / (max(||u_r||, 1e-8) * max(||c_m||, 1e-8))   (ops.Gemm, EPI_SCALE_RC)
//   3. statistics  mu[r] = mean of the K largest values of S[r, :], sd[r] = their unbiased std (ddof = 1), 2 <= K <= M.
//                  The top K is a multiset: with t the K-th largest value and g = #{v > t} the sum is
//                  sum_{v > t} v + (K - g) t.  -0.0 equals +0.0.  A NaN in the row gives mu = sd = NaN for that row only.
//   4. score       z_e = (c - mu[e]) / (sd[e] + 1e-12), z_t likewise; "z" -> z_e, "t" -> z_t, "s" -> (z_e + z_t) / 2.
//                  Not mapped through (x + 1) / 2 and not clipped.  An index outside [0, N) gives NaN for that trial.
// Conventions of the f32 strip kernels: 16-byte vectors, every guard per vector (D % 4 == 0, ld % 4 == 0), every row * ld
// in 64 bits, no atomics on global memory (integer counters in LDS only), no workgroup waits on another, fixed-order
// folds (bitwise reproducible), nothing allocated here, everything on the caller's stream.  The centring of step 1, the
// order keys of step 3, the NaN and the host's row-buffer check are defined once for all stages: trial_common.h.
#include "trial_common.h"

namespace {

// the four waves of a 256-thread workgroup, folded in wave order -> every thread holds the sum; sh: 4 doubles of LDS
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                                          // (sh may still be read from the fold before)
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// ------------------------------------------------------------------------------------------ rows_transform
// One row per wavefront, four per workgroup.  A lane transforms its vectors in f32 with the centre4 of score_pairs_kernel and
// sums their squares in double; the 64 lane sums fold through the xor butterfly.  Without length norm the transformed
// vector is stored in the same loop; with it the row is read a second time (out of the cache) once its norm is known.
constexpr int RT_WAVES = 4;

template <bool CENTER>
__device__ __forceinline__ float4 rt_load(const float* __restrict__ row, const float* __restrict__ mean,
                                          const float* __restrict__ sd, int d) {
  const float4 a = ld4(row + d);
  if constexpr (CENTER) return centre4(a, ld4(mean + d), ld4(sd + d));
  return a;
}

template <bool CENTER>
__global__ __launch_bounds__(RT_WAVES * 64) void rows_transform_kernel(const float* __restrict__ x, int64_t ld, int rows, int D,
                                                                       const float* __restrict__ mean,
                                                                       const float* __restrict__ sd, int length_norm,
                                                                       float* __restrict__ out, int64_t ld_out,
                                                                       float* __restrict__ inv_norm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * RT_WAVES + wave;
  if (r >= rows) return;                                    // (a whole wave; the kernel has no barrier)
  const float* __restrict__ row = x + r * ld;
  float* __restrict__ dst = out ? out + r * ld_out : nullptr;
  double ss = 0.0;
  for (int d = lane * 4; d < D; d += 256) {
    const float4 a = rt_load<CENTER>(row, mean, sd, d);
    ss = fma((double)a.x, (double)a.x, ss); ss = fma((double)a.y, (double)a.y, ss);
    ss = fma((double)a.z, (double)a.z, ss); ss = fma((double)a.w, (double)a.w, ss);
    if (dst && !length_norm) st4(dst + d, a.x, a.y, a.z, a.w);
  }
  ss = wave_sum_d(ss);
  double norm = sqrt(ss);
  if (length_norm) {                                        // F.normalize: u / max(||u||, 1e-12)
    const double ia = 1.0 / fmax(norm, 1e-12);
    const float f = (float)ia;
    if (dst)
      for (int d = lane * 4; d < D; d += 256) {
        const float4 a = rt_load<CENTER>(row, mean, sd, d);
        st4(dst + d, a.x * f, a.y * f, a.z * f, a.w * f);
      }
    norm *= (double)f;                                      // the norm of what was stored
  }
  if (lane == 0) inv_norm[r] = (float)(1.0 / fmax(norm, 1e-8));
}

// ------------------------------------------------------------------------------------------ topk_stats
// One workgroup per row.  A value is its order key (order_key_of, trial_common.h: the key of metrics.hip's sort, so the two
// tie the same values).  The K-th largest key by a radix select, most significant byte first: per pass a 256-bin
// histogram in LDS of the keys that match the prefix found so far, a suffix sum over the bins (one bin per thread) and the
// one bin that holds the K-th largest.  After four passes the prefix IS the key t of the K-th largest value and the
// remaining rank is K - g, the copies of t inside the top K.  Then two folds in double: sum_{v > t} v (+ (K - g) t) and
// the squares about that mean.  A row of at most TK_LDS_KEYS values is staged in LDS as keys (route 0); a longer one is
// re-read from global memory, i.e. from L2, in every pass (route 1).  Both routes give a thread the same elements in the
// same order -- vector v = tid, tid + 256, ... then the tail -- so the sums, and with them the results, are the same bits
// on either route and in every launch.
constexpr int TK_THREADS = 256, TK_LDS_KEYS = 8192;
constexpr uint32_t TK_NAN_KEY = 0xffffffffu, TK_SKIP = 256u;

template <bool STAGED, typename F>
__device__ __forceinline__ void tk_for_each(const float* __restrict__ row, const uint32_t* keys_s, int M, F&& f) {
  const int nv = M >> 2;
  for (int v = threadIdx.x; v < nv; v += TK_THREADS) {
    uint4 k;
    if constexpr (STAGED) {
      k = *reinterpret_cast<const uint4*>(keys_s + 4 * v);
    } else {
      const float4 a = ld4(row + 4 * v);
      k = make_uint4(order_key_of(a.x), order_key_of(a.y), order_key_of(a.z), order_key_of(a.w));
    }
    f(k, std::integral_constant<int, 4>{});
  }
  if ((int)threadIdx.x < (M & 3)) {                         // the tail: fewer than four values behind the last vector
    const int i = (nv << 2) + threadIdx.x;
    f(make_uint4(STAGED ? keys_s[i] : order_key_of(row[i]), 0u, 0u, 0u), std::integral_constant<int, 1>{});
  }
}

template <bool STAGED>
__global__ __launch_bounds__(TK_THREADS) void topk_stats_kernel(const float* __restrict__ S, int64_t ldS, int M, int K,
                                                                float* __restrict__ mu, float* __restrict__ sd) {
  __shared__ __attribute__((aligned(16))) uint32_t keys_s[STAGED ? TK_LDS_KEYS : 4];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wave_tot[4];
  __shared__ uint32_t chosen[2];
  __shared__ double fold_s[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = blockIdx.x;
  const float* __restrict__ row = S + r * ldS;
  if constexpr (STAGED) {
    const int nv = M >> 2;
    for (int v = tid; v < nv; v += TK_THREADS) {
      const float4 a = ld4(row + 4 * v);
      *reinterpret_cast<uint4*>(keys_s + 4 * v) = make_uint4(order_key_of(a.x), order_key_of(a.y), order_key_of(a.z), order_key_of(a.w));
    }
    if (tid < (M & 3)) keys_s[(nv << 2) + tid] = order_key_of(row[(nv << 2) + tid]);
  }
  uint32_t prefix = 0, mask = 0, k = (uint32_t)K;           // k: the rank still looked for among the keys under the prefix
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();                                        // (the staged keys are in place as well)
    int nan = 0;
    // a lane counts equal digits among its four keys once: cosines share their top bytes, and the adds to one bin of the
    // LDS are served one after the other
    tk_for_each<STAGED>(row, keys_s, M, [&](uint4 kv, auto n) {
      const uint32_t key[4] = {kv.x, kv.y, kv.z, kv.w};
      uint32_t dg[4];
#pragma unroll
      for (int a = 0; a < n.value; ++a) {
        nan |= key[a] == TK_NAN_KEY;
        dg[a] = (key[a] & mask) == prefix ? (key[a] >> shift) & 255u : TK_SKIP;
      }
#pragma unroll
      for (int a = 0; a < n.value; ++a) {
        uint32_t c = 1;
#pragma unroll
        for (int b = a + 1; b < n.value; ++b)
          if (dg[a] != TK_SKIP && dg[b] == dg[a]) { ++c; dg[b] = TK_SKIP; }
        if (dg[a] != TK_SKIP) atomicAdd(&hist[dg[a]], c);
      }
    });
    if (shift == 24) {
      if (__syncthreads_or(nan)) {                          // the whole workgroup: a NaN anywhere in the row
        if (tid == 0) { mu[r] = qnan(); sd[r] = qnan(); }
        return;
      }
    } else {
      __syncthreads();
    }
    const uint32_t h = hist[tid];
    uint32_t suf = h;                                       // keys under the prefix whose digit is >= tid
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_down(suf, o, 64);
      if (lane + o < 64) suf += y;
    }
    if (lane == 0) wave_tot[wave] = suf;
    __syncthreads();
    for (int w = wave + 1; w < 4; ++w) suf += wave_tot[w];
    if (suf >= k && suf - h < k) {                          // exactly one bin: the suffix sums fall from >= k to < k once
      chosen[0] = (uint32_t)tid;
      chosen[1] = k - (suf - h);
    }
    __syncthreads();
    prefix |= chosen[0] << shift;
    mask |= 255u << shift;
    k = chosen[1];
    __syncthreads();                                        // (hist and chosen are rewritten by the next pass)
  }
  const uint32_t tkey = prefix;                             // the K-th largest; k = K - g of its copies are in the top K
  const double t = (double)order_value_of(tkey), copies = (double)k, Kd = (double)K;
  double s = 0.0;
  tk_for_each<STAGED>(row, keys_s, M, [&](uint4 kv, auto n) {
    const uint32_t key[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
    for (int a = 0; a < n.value; ++a)
      if (key[a] > tkey) s += (double)order_value_of(key[a]);
  });
  s = block_sum_d(s, fold_s);
  const double mean = (s + copies * t) / Kd;
  double q = 0.0;
  tk_for_each<STAGED>(row, keys_s, M, [&](uint4 kv, auto n) {
    const uint32_t key[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
    for (int a = 0; a < n.value; ++a)
      if (key[a] > tkey) {
        const double d = (double)order_value_of(key[a]) - mean;
        q = fma(d, d, q);
      }
  });
  q = block_sum_d(q, fold_s);
  const double dt = t - mean;
  q += copies * (dt * dt);
  if (tid == 0) {
    mu[r] = (float)mean;
    sd[r] = (float)sqrt(q / (Kd - 1.0));
  }
}

// ------------------------------------------------------------------------------------------ score_pairs_norm
// One trial per thread: a few operations in double, rounded once.
__global__ __launch_bounds__(256) void score_pairs_norm_kernel(const float* __restrict__ cos, const int* __restrict__ pairs, int P,
                                                               const float* __restrict__ mu, const float* __restrict__ sd,
                                                               int N, int mode, float* __restrict__ score_out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int i = pairs[2 * p], j = pairs[2 * p + 1];
  if (i < 0 || i >= N || j < 0 || j >= N) {                 // not dereferenced (kept local: trial_common.h says why)
    score_out[p] = qnan();
    return;
  }
  const double c = (double)cos[p];
  const double ze = (c - (double)mu[i]) / ((double)sd[i] + 1e-12), zt = (c - (double)mu[j]) / ((double)sd[j] + 1e-12);
  score_out[p] = (float)(mode == 0 ? ze : (mode == 1 ? zt : (ze + zt) * 0.5));
}

// ------------------------------------------------------------------------------------------ segment_mean
// One workgroup per speaker and 128-dimension strip (the geometry of the f32 strip kernels: 32 feature lanes x 8 row
// lanes).  Row lane y folds rows order[begin + y], order[begin + y + 8], ... of the segment in that sequence, in double;
// the eight lanes are folded in lane order.  A segment that is empty or reaches outside `order`, or a row number outside
// [0, N), is not dereferenced: the speaker's mean comes out NaN (the host checks both before it uploads them).
using SmGeom = StripGeom<float>;

__global__ __launch_bounds__(256) void segment_mean_kernel(const float* __restrict__ bank, int64_t ld, int N, int D,
                                                           const int* __restrict__ order, const int* __restrict__ offsets,
                                                           float* __restrict__ out, int64_t ld_out) {
  __shared__ double red[SmGeom::RL][STRIP_CW];
  const int spk = blockIdx.x;
  const int cg = blockIdx.y * STRIP_CW + threadIdx.x * 4;
  const int begin = offsets[spk], end = offsets[spk + 1];
  bool bad = begin < 0 || end > N || end <= begin;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (!bad)
    for (int t = begin + (int)threadIdx.y; t < end; t += SmGeom::RL) {
      const int row = order[t];
      if (row < 0 || row >= N) { bad = true; continue; }
      if (cg < D) {
        const float4 v = ld4(bank + (int64_t)row * ld + cg);
        s[0] += (double)v.x; s[1] += (double)v.y; s[2] += (double)v.z; s[3] += (double)v.w;
      }
    }
  if (bad) s[0] = s[1] = s[2] = s[3] = (double)qnan();
  strip_put<4>(red, s);
  const int tid = threadIdx.y * SmGeom::XL + threadIdx.x;
  const int cc = blockIdx.y * STRIP_CW + tid;
  if (tid < STRIP_CW && cc < D)
    out[(int64_t)spk * ld_out + cc] = (float)(strip_lane_sum<SmGeom::RL>(red, tid) / (double)(end - begin));
}

}  // namespace

extern "C" int w2v2_rows_transform(const float* x, int64_t ld, int rows, int D, const float* mean, const float* std_,
                                   int length_norm, float* out, int64_t ld_out, float* inv_norm, void* stream) {
  W2V2_REQUIRE(rows_ok(x, ld, rows, D) && inv_norm,
               "rows_transform: bad arguments (D %% 4 == 0, ld >= D, ld %% 4 == 0, 16-byte aligned rows, inv_norm set)");
  W2V2_REQUIRE((mean == nullptr) == (std_ == nullptr), "rows_transform: mean and std are both null or both set");
  W2V2_REQUIRE(!mean || ((((uintptr_t)mean) | ((uintptr_t)std_)) & 15) == 0, "rows_transform: mean / std must be 16-byte aligned");
  W2V2_REQUIRE(out || (!mean && !length_norm), "rows_transform: out may be null only without centring and length norm");
  W2V2_REQUIRE(!out || (rows_ok(out, ld_out, rows, D) && out != x),
               "rows_transform: out is a 16-byte aligned [rows][ld_out] buffer, ld_out >= D, ld_out %% 4 == 0, not the input");
  const dim3 grid((unsigned)cdiv(rows, RT_WAVES)), block(RT_WAVES * 64);
  if (mean)
    hipLaunchKernelGGL(rows_transform_kernel<true>, grid, block, 0, as_stream(stream), x, ld, rows, D, mean, std_, length_norm, out,
                       ld_out, inv_norm);
  else
    hipLaunchKernelGGL(rows_transform_kernel<false>, grid, block, 0, as_stream(stream), x, ld, rows, D, mean, std_, length_norm, out,
                       ld_out, inv_norm);
  W2V2_CHECK_LAUNCH("rows_transform");
  return 0;
}

extern "C" int w2v2_topk_stats_lds_keys(void) { return TK_LDS_KEYS; }

extern "C" int w2v2_topk_stats(const float* S, int64_t ldS, int R, int M, int K, float* mu, float* sd, void* stream) {
  W2V2_REQUIRE(S && mu && sd && R > 0 && ((uintptr_t)S & 15) == 0 && ldS % 4 == 0,
               "topk_stats: bad arguments (a 16-byte aligned S with ldS %% 4 == 0, mu, sd, R > 0)");
  W2V2_REQUIRE(M >= 2 && M < (1 << 24) && ldS >= M, "topk_stats: M = %d outside [2, 2^24) or above ldS = %lld", M, (long long)ldS);
  W2V2_REQUIRE(K >= 2 && K <= M, "topk_stats: K = %d outside [2, M = %d]", K, M);
  const dim3 grid((unsigned)R), block(TK_THREADS);
  if (M <= TK_LDS_KEYS)
    hipLaunchKernelGGL(topk_stats_kernel<true>, grid, block, 0, as_stream(stream), S, ldS, M, K, mu, sd);
  else
    hipLaunchKernelGGL(topk_stats_kernel<false>, grid, block, 0, as_stream(stream), S, ldS, M, K, mu, sd);
  W2V2_CHECK_LAUNCH("topk_stats");
  return 0;
}

extern "C" int w2v2_score_pairs_norm(const float* cos, const int32_t* pairs, int P, const float* mu, const float* sd, int N,
                                     int mode, float* score_out, void* stream) {
  W2V2_REQUIRE(cos && pairs && mu && sd && score_out && P > 0 && N > 0, "score_pairs_norm: bad arguments");
  W2V2_REQUIRE(mode >= 0 && mode <= 2, "score_pairs_norm: mode %d is not 0 (z), 1 (t) or 2 (s)", mode);
  hipLaunchKernelGGL(score_pairs_norm_kernel, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, as_stream(stream), cos, pairs, P, mu, sd,
                     N, mode, score_out);
  W2V2_CHECK_LAUNCH("score_pairs_norm");
  return 0;
}

extern "C" int w2v2_segment_mean(const float* bank, int64_t ld, int N, int D, const int32_t* order, const int32_t* offsets,
                                 int S, float* out, int64_t ld_out, void* stream) {
  W2V2_REQUIRE(rows_ok(bank, ld, N, D) && order && offsets,
               "segment_mean: bad arguments (D %% 4 == 0, ld >= D, ld %% 4 == 0, 16-byte aligned bank)");
  W2V2_REQUIRE(S >= 1 && S <= N && cdiv(D, STRIP_CW) <= 65535, "segment_mean: S = %d segments outside [1, N = %d]", S, N);
  W2V2_REQUIRE(out && ld_out >= D, "segment_mean: out is [S][ld_out], ld_out >= D");
  hipLaunchKernelGGL(segment_mean_kernel, dim3((unsigned)S, (unsigned)cdiv(D, STRIP_CW)), dim3(SmGeom::XL, SmGeom::RL), 0,
                     as_stream(stream), bank, ld, N, D, order, offsets, out, ld_out);
  W2V2_CHECK_LAUNCH("segment_mean");
  return 0;
}
