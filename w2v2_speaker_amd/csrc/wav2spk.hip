// wav2spk.hip -- the non-GEMM pieces of the wav2spk path (ref: src/lightning_modules/speaker/wav2spk.py:116-299,
// src/layers/temporal_gating.py; the host layer is w2v2_speaker_amd/wav2spk.py).
//
//   encoder layer  = Conv1d(bias, zero padding, stride) -> InstanceNorm1d(no affine, biased variance over time per
//                    utterance and channel, eps 1e-5) -> ReLU
//   layer 0        = w2v2_conv1d_first: Cin = 1, straight from the waveform (no im2col: k = 10 taps per output)
//   layers 1-4,
//   aggregator     = w2v2_im2col_zero (taps gathered with zero padding, channels-last: tap_gather.h with PadZero,
//                    dilation 1) + the exact-f32 GEMM (gemm_f32*.hip); w2v2_col2im_zero is the exact adjoint of the gather,
//                    itself a gather (one writer per element; tap_gather.h)
//   temporal gate  = y = sigmoid(P) * x, P = X W^T + b a plain GEMM
//   bias, ReLU     = w2v2_sum_bias_act_rows: the K range of a long convolution is cut into chunks (one batched GEMM), whose
//                    partial products this kernel adds in a fixed order with the bias (and the aggregator's ReLU)
//
// f32 only, channels-last [B*T][C] with a row stride.  A thread owns ONE 16-byte vector of 4 channels and every guard is per
// vector (the bn_align rule of tdnn.hip), so C = 40, 200, 300 and 512 run unpadded.  No atomics; every reduction has a
// fixed order, so every result is bitwise reproducible.  The statistics blocks are IN_FB frames of ONE utterance, counted
// from its first frame -- never a function of T -- so a row of a padded batch (lens) equals the utterance run alone.
// Variable-length forms (lens: device int32 [B]): every stage writes ZEROS into the rows past an utterance's own frame
// count; those zeros are the zero padding of the next layer's gather, which therefore needs no lengths itself.
#include "tap_gather.h"

using InGeom = StripGeom<float>;       // the InstanceNorm workgroups: 32 channel lanes x 4 channels, 8 row lanes
constexpr int IN_FB = 128;             // frames per statistics block
constexpr int IN_RPT = IN_FB / InGeom::RL;  // rows per thread: all 16 in flight (64 registers)
constexpr int C1_ROWS = 256;           // rows per partial block of the layer-0 weight gradient

// ------------------------------------------------------------------------------------------ layer 0: Cin = 1
// z[b][t][c] = bias[c] + sum_j w[c][j] * x[b][t * stride + j - pad], x = 0 outside [0, n_b).  lens = SAMPLES per utterance:
// utterance b then has (n_b + 2 pad - k) / stride + 1 frames and the rows past them are written as zeros.
template <bool LEN>
__global__ void conv1d_first_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                    const float* __restrict__ bias, float* __restrict__ z, int64_t ldz, int B, int N, int T,
                                    int C, int k, int stride, int pad, LensArg<LEN> lens) {
  const int C4 = C >> 2;
  const int64_t total = (int64_t)B * T * C4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    const int64_t row = i / C4;
    const int b = (int)(row / T), t = (int)(row % T);
    int nb = N;
    float* dst = z + row * ldz + c;
    if constexpr (LEN) {
      nb = min(lens[b], N);
      if (t >= (nb + 2 * pad - k) / stride + 1) {
        st4(dst, 0.f, 0.f, 0.f, 0.f);
        continue;
      }
    }
    const float4 bv = ld4(bias + c);
    float acc[4] = {bv.x, bv.y, bv.z, bv.w};
    const float* xb = x + (int64_t)b * ldx;
    const int p0 = t * stride - pad;
    for (int j = 0; j < k; ++j) {
      const int p = p0 + j;
      const float xv = (p >= 0 && p < nb) ? xb[p] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(w[(c + e) * k + j], xv, acc[e]);
    }
    st4(dst, acc[0], acc[1], acc[2], acc[3]);
  }
}
// dW[c][j] = sum_{b,t} dz[b][t][c] * x[b][t * stride + j - pad]: every workgroup folds C1_ROWS rows into one partial row
// [k][C] (row order), the fold kernel adds the partial rows in block order, in double
__global__ __launch_bounds__(256) void conv1d_first_bwd_partial_kernel(const float* __restrict__ x, int64_t ldx,
                                                                       const float* __restrict__ dz, int64_t lddz,
                                                                       float* __restrict__ partial, int B, int N, int T,
                                                                       int C, int k, int stride, int pad) {
  const int64_t M = (int64_t)B * T;
  const int64_t r0 = (int64_t)blockIdx.x * C1_ROWS, r1 = min(M, r0 + C1_ROWS);
  for (int e = threadIdx.x; e < C * k; e += 256) {
    const int j = e / C, c = e - j * C;
    float acc = 0.f;
    for (int64_t row = r0; row < r1; ++row) {
      const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
      const int p = t * stride + j - pad;
      if (p >= 0 && p < N) acc = fmaf(dz[row * lddz + c], x[(int64_t)b * ldx + p], acc);
    }
    partial[(int64_t)blockIdx.x * C * k + e] = acc;
  }
}
__global__ void conv1d_first_bwd_fold_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ dw, int C,
                                             int k) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= C * k) return;
  double s = 0.0;
  for (int i = 0; i < nblk; ++i) s += (double)partial[(int64_t)i * C * k + e];
  const int j = e / C, c = e - j * C;
  dw[c * k + j] += (float)s;
}

// ------------------------------------------------------------------------------------------ InstanceNorm1d + ReLU
// Two launches per direction, the shape of tdnn.hip's BatchNorm pair with the statistics per (utterance, channel).
// (1) partial: a workgroup takes IN_FB frames of one utterance and a 128-channel strip and writes, per channel, the block's
// mean (as an f32 pair: the half ulp of an f32 mean is 1e-5 of a standard deviation 300 times smaller than the mean) and its
// CENTRED second moment sum (z - mean_block)^2: the sums run in double, so the mean of a constant channel is that constant
// exactly and a large DC component costs the variance nothing (E[z^2] - mean^2 would lose mean^2 / var digits).
// (2) apply: every workgroup first combines the blocks of ITS utterance and strip in double, in block order (Chan et al.:
// M2 += M2_j + delta^2 n n_j / (n + n_j)) -- the same numbers in every workgroup -- then walks its rows.  The workgroups
// of block 0 publish mean / rstd.
template <bool LEN>
__global__ __launch_bounds__(256) void in_partial_kernel(const float* __restrict__ z, int64_t ldz,
                                                         float* __restrict__ partial, int T, int C, int nblk,
                                                         LensArg<LEN> lens) {
  __shared__ double red[InGeom::RL][STRIP_CW];
  __shared__ float mu_s[STRIP_CW];
  const int b = blockIdx.z, blk = blockIdx.y;
  int Tb = T;
  if constexpr (LEN) Tb = min(lens[b], T);
  const int t0 = blk * IN_FB;
  if (t0 >= Tb) return;                                   // (the whole workgroup: no barrier is skipped by a part of it)
  const int n = min(IN_FB, Tb - t0);
  const int cg = blockIdx.x * STRIP_CW + threadIdx.x * 4;
  const int tid = threadIdx.y * InGeom::XL + threadIdx.x;
  double mean_d, m2;
  strip_centred_moments<IN_RPT>(z + ((int64_t)b * T + t0) * ldz + cg, ldz, n, cg < C, red, mu_s, mean_d, m2);
  const int cc = blockIdx.x * STRIP_CW + tid;
  if (tid < STRIP_CW && cc < C) {                         // the block mean as an f32 pair (centre + remainder)
    float* dst = partial + (((int64_t)b * nblk + blk) * C + cc) * 4;
    dst[0] = mu_s[tid];
    dst[1] = (float)(mean_d - (double)mu_s[tid]);
    dst[2] = (float)m2;
    dst[3] = 0.f;
  }
}
// mean / rstd of channel cc of utterance b from its block partials, in double, in block order; the mean as an f32 pair
// mu + mu_lo: z - mean is formed as (z - mu) - mu_lo, so the half ulp of an f32 mean -- 1e-7 of a DC component, i.e.
// 1e-5 of a standard deviation 300 times smaller -- does not reach the normalised output
__device__ __forceinline__ void in_combine(const float* __restrict__ partial, int b, int nblk, int C, int cc, int Tb, float eps,
                                           float& mu, float& mu_lo, float& rstd) {
  double mean = 0.0, m2 = 0.0, cnt = 0.0;
  const int nb = (Tb + IN_FB - 1) / IN_FB;
  for (int j = 0; j < nb; ++j) {
    const float4 src = ld4(partial + (((int64_t)b * nblk + j) * C + cc) * 4);
    const double nj = (double)min(IN_FB, Tb - j * IN_FB), mj = (double)src.x + (double)src.y, qj = (double)src.z;
    const double delta = mj - mean, tot = cnt + nj;
    mean += delta * nj / tot;
    m2 += qj + delta * delta * cnt * nj / tot;
    cnt = tot;
  }
  mu = (float)mean;
  mu_lo = (float)(mean - (double)mu);
  rstd = (float)(1.0 / sqrt(m2 / (double)Tb + (double)eps));
}
template <bool LEN>
__global__ __launch_bounds__(256) void in_apply_kernel(const float* __restrict__ z, int64_t ldz,
                                                       const float* __restrict__ partial, int nblk,
                                                       float* __restrict__ mean_rstd, float* __restrict__ y, int64_t ldy,
                                                       int T, int C, float eps, LensArg<LEN> lens) {
  __shared__ float cf[3][STRIP_CW];                          // mean, rstd, the mean's low part
  const int b = blockIdx.z, blk = blockIdx.y;
  int Tb = T;
  if constexpr (LEN) Tb = min(lens[b], T);
  const int t0 = blk * IN_FB, t1 = min(T, t0 + IN_FB);
  const int cl = threadIdx.x * 4, cg = blockIdx.x * STRIP_CW + cl;
  const int tid = threadIdx.y * InGeom::XL + threadIdx.x;
  const int cc = blockIdx.x * STRIP_CW + tid;
  if (t0 < Tb) {
    if (tid < STRIP_CW && cc < C) {
      float mu, mu_lo, rstd;
      in_combine(partial, b, nblk, C, cc, Tb, eps, mu, mu_lo, rstd);
      cf[0][tid] = mu;
      cf[1][tid] = rstd;
      cf[2][tid] = mu_lo;
      if (blk == 0) {
        mean_rstd[((int64_t)b * C + cc) * 2] = mu;
        mean_rstd[((int64_t)b * C + cc) * 2 + 1] = rstd;
      }
    }
    __syncthreads();                                      // (t0 < Tb is uniform over the workgroup)
  }
  if (cg >= C) return;
  for (int t = t0 + threadIdx.y; t < t1; t += InGeom::RL) {
    float* dst = y + ((int64_t)b * T + t) * ldy + cg;
    if (t >= Tb) {
      st4(dst, 0.f, 0.f, 0.f, 0.f);
      continue;
    }
    const float4 v = ld4(z + ((int64_t)b * T + t) * ldz + cg);
    const float zz[4] = {v.x, v.y, v.z, v.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fmaxf(((zz[e] - cf[0][cl + e]) - cf[2][cl + e]) * cf[1][cl + e], 0.f);
    st4(dst, o[0], o[1], o[2], o[3]);
  }
}
// backward: g = dy where y > 0, else 0; zhat = (z - mean) rstd; dz = rstd (g - mean_t g - zhat mean_t (g zhat)).
// partial: per block the two sums (f32 per thread and row lane, fixed order); apply: the blocks in double, in block order.
__global__ __launch_bounds__(256) void in_bwd_partial_kernel(const float* __restrict__ dy, int64_t lddy,
                                                             const float* __restrict__ z, int64_t ldz,
                                                             const float* __restrict__ y, int64_t ldy,
                                                             const float* __restrict__ mean_rstd,
                                                             float* __restrict__ partial, int T, int C, int nblk) {
  __shared__ float red[InGeom::RL][STRIP_CW][2];
  const int b = blockIdx.z, blk = blockIdx.y;
  const int t0 = blk * IN_FB, t1 = min(T, t0 + IN_FB);
  const int cg = blockIdx.x * STRIP_CW + threadIdx.x * 4;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  if (cg < C) {
    float mu[4], rs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      mu[e] = mean_rstd[((int64_t)b * C + cg + e) * 2];
      rs[e] = mean_rstd[((int64_t)b * C + cg + e) * 2 + 1];
    }
    for (int t = t0 + threadIdx.y; t < t1; t += InGeom::RL) {
      const int64_t row = (int64_t)b * T + t;
      const float4 gv = ld4(dy + row * lddy + cg), zv = ld4(z + row * ldz + cg), yv = ld4(y + row * ldy + cg);
      const float g[4] = {yv.x > 0.f ? gv.x : 0.f, yv.y > 0.f ? gv.y : 0.f, yv.z > 0.f ? gv.z : 0.f, yv.w > 0.f ? gv.w : 0.f};
      const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s1[e] += g[e];
        s2[e] = fmaf(g[e], (zz[e] - mu[e]) * rs[e], s2[e]);
      }
    }
  }
  strip_store_partial2<4>(red, s1, s2, partial, (int64_t)b * nblk + blk, C);
}
__global__ __launch_bounds__(256) void in_bwd_apply_kernel(const float* __restrict__ dy, int64_t lddy,
                                                           const float* __restrict__ z, int64_t ldz,
                                                           const float* __restrict__ y, int64_t ldy,
                                                           const float* __restrict__ mean_rstd,
                                                           const float* __restrict__ partial, int nblk,
                                                           float* __restrict__ dz, int64_t lddz, int T, int C) {
  __shared__ float cf[4][STRIP_CW];                          // mean, rstd, mean_t g, mean_t (g zhat)
  const int b = blockIdx.z, blk = blockIdx.y;
  const int t0 = blk * IN_FB, t1 = min(T, t0 + IN_FB);
  const int cl = threadIdx.x * 4, cg = blockIdx.x * STRIP_CW + cl;
  const int tid = threadIdx.y * InGeom::XL + threadIdx.x;
  const int cc = blockIdx.x * STRIP_CW + tid;
  if (tid < STRIP_CW && cc < C) {
    double a1 = 0.0, a2 = 0.0;
    for (int j = 0; j < nblk; ++j) {
      const float* src = partial + (((int64_t)b * nblk + j) * C + cc) * 2;
      a1 += (double)src[0];
      a2 += (double)src[1];
    }
    cf[0][tid] = mean_rstd[((int64_t)b * C + cc) * 2];
    cf[1][tid] = mean_rstd[((int64_t)b * C + cc) * 2 + 1];
    cf[2][tid] = (float)(a1 / T);
    cf[3][tid] = (float)(a2 / T);
  }
  __syncthreads();
  if (cg >= C) return;
  for (int t = t0 + threadIdx.y; t < t1; t += InGeom::RL) {
    const int64_t row = (int64_t)b * T + t;
    const float4 gv = ld4(dy + row * lddy + cg), zv = ld4(z + row * ldz + cg), yv = ld4(y + row * ldy + cg);
    const float g[4] = {yv.x > 0.f ? gv.x : 0.f, yv.y > 0.f ? gv.y : 0.f, yv.z > 0.f ? gv.z : 0.f, yv.w > 0.f ? gv.w : 0.f};
    const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float rs = cf[1][cl + e], zh = (zz[e] - cf[0][cl + e]) * rs;
      o[e] = rs * (g[e] - cf[2][cl + e] - zh * cf[3][cl + e]);
    }
    st4(dz + row * lddz + cg, o[0], o[1], o[2], o[3]);
  }
}

// ------------------------------------------------------------------------------------------ temporal gate, row ReLU
// y = sigmoid(p) * x over n / 4 vectors
__global__ void gate_fwd_kernel(const float* __restrict__ p, const float* __restrict__ x, float* __restrict__ y, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 pv = ld4(p + 4 * i), xv = ld4(x + 4 * i);
    st4(y + 4 * i, sigmoid_f(pv.x) * xv.x, sigmoid_f(pv.y) * xv.y, sigmoid_f(pv.z) * xv.z, sigmoid_f(pv.w) * xv.w);
  }
}
// dp = dy * x * s (1 - s), dx = dy * s (the direct part; the caller adds dp W)
__global__ void gate_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ p, const float* __restrict__ x,
                                float* __restrict__ dp, float* __restrict__ dx, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 gv = ld4(dy + 4 * i), pv = ld4(p + 4 * i), xv = ld4(x + 4 * i);
    const float s[4] = {sigmoid_f(pv.x), sigmoid_f(pv.y), sigmoid_f(pv.z), sigmoid_f(pv.w)};
    const float g[4] = {gv.x, gv.y, gv.z, gv.w}, xx[4] = {xv.x, xv.y, xv.z, xv.w};
    float a[4], d[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = g[e] * xx[e] * (s[e] * (1.0f - s[e]));
      d[e] = g[e] * s[e];
    }
    st4(dp + 4 * i, a[0], a[1], a[2], a[3]);
    st4(dx + 4 * i, d[0], d[1], d[2], d[3]);
  }
}
// y[b][t][c] = act(bias[c] + ((p_0 + p_1) + ... + p_{S-1})[b][t][c]) for t < lens[b] (all rows without lens), zeros past it:
// the fixed-order fold of the S partial products of a convolution whose K range was cut into S chunks (an f32 chain of
// K = 1536 fmas loses 2.6 times what torch's blocked f32 sum does; chunks of <= 128 folded in double lose no more than it),
// the bias, and the aggregator's ReLU.  bias may be null, S may be 1, y may be p_0.
template <bool LEN>
__global__ void sum_bias_act_rows_kernel(const float* __restrict__ parts, int S, int64_t part_stride,
                                         const float* __restrict__ bias, float* __restrict__ y, int B, int T, int C, int relu,
                                         LensArg<LEN> lens) {
  const int C4 = C >> 2;
  const int64_t total = (int64_t)B * T * C4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (LEN) {
      const int64_t row = i / C4;
      const int b = (int)(row / T), t = (int)(row % T);
      if (t >= lens[b]) {
        st4(y + 4 * i, 0.f, 0.f, 0.f, 0.f);
        continue;
      }
    }
    float4 a = ld4(parts + 4 * i);
    if (S > 1 || bias != nullptr) {                       // the fold runs in double: it adds one rounding, the last
      double d[4] = {(double)a.x, (double)a.y, (double)a.z, (double)a.w};
      for (int q = 1; q < S; ++q) {
        const float4 v = ld4(parts + q * part_stride + 4 * i);
        d[0] += (double)v.x; d[1] += (double)v.y; d[2] += (double)v.z; d[3] += (double)v.w;
      }
      if (bias != nullptr) {
        const float4 bv = ld4(bias + (int)(i % C4) * 4);
        d[0] += (double)bv.x; d[1] += (double)bv.y; d[2] += (double)bv.z; d[3] += (double)bv.w;
      }
      a = make_float4((float)d[0], (float)d[1], (float)d[2], (float)d[3]);
    }
    if (relu) { a.x = fmaxf(a.x, 0.f); a.y = fmaxf(a.y, 0.f); a.z = fmaxf(a.z, 0.f); a.w = fmaxf(a.w, 0.f); }
    st4(y + 4 * i, a.x, a.y, a.z, a.w);
  }
}

// ------------------------------------------------------------------------------------------ C ABI
static bool conv_geom_ok(int Tin, int Tout, int k, int stride, int pad) {
  return Tin > 0 && k > 0 && stride > 0 && pad >= 0 && pad < k && Tin + 2 * pad >= k && Tout == (Tin + 2 * pad - k) / stride + 1;
}

extern "C" int w2v2_conv1d_first(const float* x, int64_t ldx, const float* w, const float* bias, float* z, int64_t ldz,
                                 const int* lens, int B, int N, int T, int C, int k, int stride, int pad, void* stream) {
  W2V2_REQUIRE(x && w && bias && z && B > 0 && C > 0 && C % 4 == 0 && ldz >= C && ldz % 4 == 0 && ldx >= N &&
                   conv_geom_ok(N, T, k, stride, pad),
               "conv1d_first: bad arguments (C, ldz multiples of 4; T = (N + 2 pad - k) / stride + 1)");
  const int nb = blocks256((int64_t)B * T * (C >> 2));
  hipStream_t st = as_stream(stream);
  W2V2_DISPATCH_LEN(lens, hipLaunchKernelGGL(conv1d_first_kernel<LEN>, dim3(nb), dim3(256), 0, st, x, ldx, w, bias, z, ldz,
                                             B, N, T, C, k, stride, pad, lens));
  W2V2_CHECK_LAUNCH("conv1d_first");
  return 0;
}
extern "C" int w2v2_conv1d_first_bwd_workspace_floats(int M, int C, int k) { return (int)cdiv(M, C1_ROWS) * C * k; }
extern "C" int w2v2_conv1d_first_bwd(const float* x, int64_t ldx, const float* dz, int64_t lddz, float* workspace, float* dw,
                                     int B, int N, int T, int C, int k, int stride, int pad, void* stream) {
  W2V2_REQUIRE(x && dz && workspace && dw && B > 0 && C > 0 && lddz >= C && ldx >= N && conv_geom_ok(N, T, k, stride, pad),
               "conv1d_first_bwd: bad arguments");
  const int nblk = (int)cdiv((int64_t)B * T, C1_ROWS);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(conv1d_first_bwd_partial_kernel, dim3(nblk), dim3(256), 0, st, x, ldx, dz, lddz, workspace, B, N, T, C,
                     k, stride, pad);
  hipLaunchKernelGGL(conv1d_first_bwd_fold_kernel, dim3((unsigned)cdiv(C * k, 256)), dim3(256), 0, st, workspace, nblk, dw,
                     C, k);
  W2V2_CHECK_LAUNCH("conv1d_first_bwd");
  return 0;
}

extern "C" int w2v2_im2col_zero(const float* x, int64_t ldx, float* col, int B, int Tin, int Tout, int Cin, int k,
                                int stride, int pad, void* stream) {
  W2V2_REQUIRE(x && col && B > 0 && Cin > 0 && Cin % 4 == 0 && ldx >= Cin && ldx % 4 == 0 &&
                   conv_geom_ok(Tin, Tout, k, stride, pad),
               "im2col_zero: bad arguments (Cin, ldx multiples of 4; Tout = (Tin + 2 pad - k) / stride + 1)");
  return tap_gather_launch<float, PadZero, false>("im2col_zero", x, ldx, nullptr, 0, col, nullptr,
                                                  TapGeom{B, Tin, Tout, Cin, k, stride, 1, pad}, stream);
}
extern "C" int w2v2_col2im_zero(const float* dcol, float* dx, int64_t lddx, int B, int Tin, int Tout, int Cin, int k,
                                int stride, int pad, void* stream) {
  W2V2_REQUIRE(dcol && dx && B > 0 && Cin > 0 && Cin % 4 == 0 && lddx >= Cin && lddx % 4 == 0 &&
                   conv_geom_ok(Tin, Tout, k, stride, pad),
               "col2im_zero: bad arguments (Cin, lddx multiples of 4; Tout = (Tin + 2 pad - k) / stride + 1)");
  const TapGeom g{B, Tin, Tout, Cin, k, stride, 1, pad};
  return stride == 1 ? tap_adjoint_launch<float, PadZero, true>("col2im_zero", dcol, dx, lddx, g, 0, stream)   // the aggregator
                     : tap_adjoint_launch<float, PadZero, false>("col2im_zero", dcol, dx, lddx, g, 0, stream);
}

// forward: {mean, its low part, centred squares, 0} per (utterance, block, channel); backward: two sums
extern "C" int w2v2_instnorm_workspace_floats(int B, int T, int C) { return B * (int)cdiv(T, IN_FB) * C * 4; }
extern "C" int w2v2_instnorm_relu_fwd(const float* z, int64_t ldz, float* workspace, float* mean_rstd, float* y, int64_t ldy,
                                      const int* lens, int B, int T, int C, float eps, void* stream) {
  W2V2_REQUIRE(z && workspace && mean_rstd && y && B > 0 && B <= 65535 && T > 0 && C > 0 && C % 4 == 0 && ldz >= C &&
                   ldz % 4 == 0 && ldy >= C && ldy % 4 == 0,
               "instnorm_relu_fwd: bad arguments (C and the row strides multiples of 4, B <= 65535)");
  const int nblk = (int)cdiv(T, IN_FB);
  const dim3 grid((unsigned)cdiv(C, STRIP_CW), nblk, B), block(InGeom::XL, InGeom::RL);
  hipStream_t st = as_stream(stream);
  W2V2_DISPATCH_LEN(lens,
    hipLaunchKernelGGL(in_partial_kernel<LEN>, grid, block, 0, st, z, ldz, workspace, T, C, nblk, lens);
    hipLaunchKernelGGL(in_apply_kernel<LEN>, grid, block, 0, st, z, ldz, workspace, nblk, mean_rstd, y, ldy, T, C, eps, lens));
  W2V2_CHECK_LAUNCH("instnorm_relu_fwd");
  return 0;
}
extern "C" int w2v2_instnorm_relu_bwd(const float* dy, int64_t lddy, const float* z, int64_t ldz, const float* y, int64_t ldy,
                                      const float* mean_rstd, float* workspace, float* dz, int64_t lddz, int B, int T, int C,
                                      void* stream) {
  W2V2_REQUIRE(dy && z && y && mean_rstd && workspace && dz && B > 0 && B <= 65535 && T > 0 && C > 0 && C % 4 == 0 &&
                   lddy >= C && lddy % 4 == 0 && ldz >= C && ldz % 4 == 0 && ldy >= C && ldy % 4 == 0 && lddz >= C &&
                   lddz % 4 == 0,
               "instnorm_relu_bwd: bad arguments (C and the row strides multiples of 4, B <= 65535)");
  const int nblk = (int)cdiv(T, IN_FB);
  const dim3 grid((unsigned)cdiv(C, STRIP_CW), nblk, B), block(InGeom::XL, InGeom::RL);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(in_bwd_partial_kernel, grid, block, 0, st, dy, lddy, z, ldz, y, ldy, mean_rstd, workspace, T, C, nblk);
  hipLaunchKernelGGL(in_bwd_apply_kernel, grid, block, 0, st, dy, lddy, z, ldz, y, ldy, mean_rstd, workspace, nblk, dz, lddz,
                     T, C);
  W2V2_CHECK_LAUNCH("instnorm_relu_bwd");
  return 0;
}

extern "C" int w2v2_gate_fwd(const float* p, const float* x, float* y, int64_t n, void* stream) {
  W2V2_REQUIRE(p && x && y && n > 0 && n % 4 == 0, "gate_fwd: bad arguments (n a multiple of 4)");
  hipLaunchKernelGGL(gate_fwd_kernel, dim3(blocks256(n >> 2)), dim3(256), 0, as_stream(stream), p, x, y, n >> 2);
  W2V2_CHECK_LAUNCH("gate_fwd");
  return 0;
}
extern "C" int w2v2_gate_bwd(const float* dy, const float* p, const float* x, float* dp, float* dx, int64_t n, void* stream) {
  W2V2_REQUIRE(dy && p && x && dp && dx && n > 0 && n % 4 == 0, "gate_bwd: bad arguments (n a multiple of 4)");
  hipLaunchKernelGGL(gate_bwd_kernel, dim3(blocks256(n >> 2)), dim3(256), 0, as_stream(stream), dy, p, x, dp, dx, n >> 2);
  W2V2_CHECK_LAUNCH("gate_bwd");
  return 0;
}
extern "C" int w2v2_sum_bias_act_rows(const float* parts, int S, int64_t part_stride, const float* bias, float* y,
                                      const int* lens, int B, int T, int C, int relu, void* stream) {
  W2V2_REQUIRE(parts && y && S >= 1 && B > 0 && T > 0 && C > 0 && C % 4 == 0 && (S == 1 || part_stride >= (int64_t)B * T * C) &&
                   part_stride % 4 == 0,
               "sum_bias_act_rows: bad arguments (C and part_stride multiples of 4, part_stride >= B * T * C)");
  const int nb = blocks256((int64_t)B * T * (C >> 2));
  hipStream_t st = as_stream(stream);
  W2V2_DISPATCH_LEN(lens, hipLaunchKernelGGL(sum_bias_act_rows_kernel<LEN>, dim3(nb), dim3(256), 0, st, parts, S, part_stride,
                                             bias, y, B, T, C, relu, lens));
  W2V2_CHECK_LAUNCH("sum_bias_act_rows");
  return 0;
}
