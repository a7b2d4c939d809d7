// tdnn.hip -- the non-GEMM pieces of the ECAPA-TDNN path (BASELINE configs[4];
// ref: src/lightning_modules/speaker/ecapa_tdnn.py:75-85 -> speechbrain 0.5.x ECAPA_TDNN, restated in
// oracle/ecapa_oracle.py -- speechbrain is not part of the reference tree: parity unpinned).
//
//   TDNNBlock  = Conv1d("same", reflect padding, dilation) -> ReLU -> BatchNorm1d (batch statistics)
//   conv       = im2col_reflect (taps gathered with reflection, channels-last: tap_gather.h with PadReflect, stride 1) +
//                GEMM (gemm.hip) [k = 1: GEMM only]; col2im_reflect is the adjoint of the gather (tap_gather.h)
//   SE block   = mean_t -> Linear -> ReLU -> Linear -> sigmoid -> per-(utterance, channel) gate
//   Res2Net    = channel slices of one [B*T, C] tensor (row-strided views) with cumulative adds
// and of the x-vector path (xvector.py; ref: src/lightning_modules/speaker/xvector.py -> speechbrain 0.5.x Xvector, as
// recollected): its TDNN block is Conv1d -> LeakyReLU(0.01) -> BatchNorm1d (the `act` mode of the BatchNorm kernels), its
// pooling the plain statistics pooling below (w2v2_stat_pool_*).
//
// Everything here is HBM-bound elementwise / reduction work over channels-last [B*T, C] activations; reductions
// over rows are two-stage with a fixed order (deterministic, no atomics).  Row-strided operands (ld*) let the
// Res2Net slices and the MFA concatenation live inside their parent tensors without copies.
#include "tap_gather.h"

constexpr int BN_AROWS = 256;     // rows one workgroup of the apply kernels walks (64 where that leaves CUs idle: bn_arows)

// ------------------------------------------------------------------------------------------ BatchNorm (+ReLU)
// Two launches per direction.  (1) partial: every workgroup reduces `rows` rows of a 128-channel strip to one
// (sum, sum of squares) pair per channel -- 16-byte loads, 16 row lanes, an LDS fold in a fixed order.  (2) apply:
// every workgroup first folds the partial blocks of ITS 128 channels (a few tens of KiB out of L2, in double, in
// block order -- the same numbers in every workgroup, so the result does not depend on the grid), then walks its
// rows.  The workgroups of row-block 0 publish mean / rstd (the backward reads them), update the running
// statistics, and in the backward write dgamma / dbeta.  No finalize launch, no atomics, no grid-wide fence.
// The activation in front of the statistics (`act`, W2V2_BN_ACT_*): 0 none, 1 ReLU (ECAPA's TDNNBlock), 2 LeakyReLU with
// slope 0.01 (the x-vector blocks: conv -> LeakyReLU -> BatchNorm).  The backward multiplies by 1 where the saved
// pre-activation is > 0 and by 0 / the slope elsewhere (torch's convention at a == 0).
constexpr int BN_ACT_RELU = 1, BN_ACT_LEAKY = 2;
constexpr float BN_LEAKY_SLOPE = 0.01f;
__device__ __forceinline__ float bn_act(float v, int act) {
  return act == BN_ACT_RELU ? fmaxf(v, 0.f) : (act == BN_ACT_LEAKY && !(v > 0.f)) ? BN_LEAKY_SLOPE * v : v;
}
constexpr int BN_PROWS = 256;     // rows per partial-sum block

template <typename T>
__global__ __launch_bounds__(256) void bn_partial_kernel(const T* __restrict__ a, int64_t lda,
                                                         float* __restrict__ partial, int M, int C, int act) {
  __shared__ float red[STRIP_RL_MAX][STRIP_CW][2];
  using G = StripGeom<T>;
  constexpr int EPT = G::EPT, RL = G::RL, UN = G::UN;
  const int cg = blockIdx.x * STRIP_CW + threadIdx.x * EPT;
  const int m0 = blockIdx.y * BN_PROWS, m1 = min(M, m0 + BN_PROWS);
  float s1[EPT] = {}, s2[EPT] = {};
  if (cg < C)
    for (int m = m0 + threadIdx.y; m < m1; m += UN * RL) {      // UN independent 16-byte loads in flight
      typename G::Vec v[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) v[u].load(a + (int64_t)min(m + u * RL, m1 - 1) * lda + cg);
#pragma unroll
      for (int u = 0; u < UN; ++u)
        if (m + u * RL < m1) {
#pragma unroll
          for (int e = 0; e < EPT; ++e) {
            const float r = bn_act(v[u].v[e], act);
            s1[e] += r;
            s2[e] = fmaf(r, r, s2[e]);
          }
        }
    }
  strip_store_partial2<EPT>(red, s1, s2, partial, (int64_t)blockIdx.y, C);
}
// the two column sums of channel blockIdx.x*128 + (tid & 127), folded over the partial blocks in a fixed order: wave g
// takes blocks g, g+4, ... (one 16-byte load = 2 channels x 2 sums per lane, four loads in flight), then the four
// wave results are added in wave order
__device__ __forceinline__ void bn_fold(const float* __restrict__ partial, int nblk, int C, double (*fold)[STRIP_CW][2],
                                        double& s1, double& s2, int tid) {
  const int q = tid & 63, grp = tid >> 6;
  const int cq = blockIdx.x * STRIP_CW + 2 * q;
  double p[4] = {0.0, 0.0, 0.0, 0.0};
  if (cq < C) {
    const float* src = partial + (int64_t)cq * 2;
    int j = grp;
    for (; j + 12 < nblk; j += 16) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(src + (int64_t)(j + 4 * u) * C * 2);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        p[0] += (double)v[u].x; p[1] += (double)v[u].y; p[2] += (double)v[u].z; p[3] += (double)v[u].w;
      }
    }
    for (; j < nblk; j += 4) {
      const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)j * C * 2);
      p[0] += (double)v.x; p[1] += (double)v.y; p[2] += (double)v.z; p[3] += (double)v.w;
    }
  }
  fold[grp][2 * q][0] = p[0];
  fold[grp][2 * q][1] = p[1];
  fold[grp][2 * q + 1][0] = p[2];
  fold[grp][2 * q + 1][1] = p[3];
  __syncthreads();
  const int c = tid & (STRIP_CW - 1);
  s1 = ((fold[0][c][0] + fold[1][c][0]) + fold[2][c][0]) + fold[3][c][0];
  s2 = ((fold[0][c][1] + fold[1][c][1]) + fold[2][c][1]) + fold[3][c][1];
}
// mode 1: batch statistics from `partial` (training); mode 0: the running statistics (BatchNorm1d.eval())
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ a, int64_t lda,
                                                       const float* __restrict__ partial, int nblk,
                                                       float* __restrict__ mean_rstd, float* __restrict__ running,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       T* __restrict__ y, int64_t ldy, int M, int C, int act,
                                                       float eps, float momentum, int mode, int arows) {
  __shared__ double fold[4][STRIP_CW][2];
  __shared__ float cf[4][STRIP_CW];                 // mean, rstd, gamma, beta of the strip
  using G = StripGeom<T>;
  constexpr int EPT = G::EPT, RL = G::RL, UN = G::UN;
  const int tid = threadIdx.y * G::XL + threadIdx.x;
  const int c = tid & (STRIP_CW - 1), cc = blockIdx.x * STRIP_CW + c;
  float mu = 0.f, rstd = 0.f;
  if (mode) {
    double s1, s2;
    bn_fold(partial, nblk, C, fold, s1, s2, tid);
    const double mud = s1 / M;
    double var = s2 / M - mud * mud;
    var = var > 0.0 ? var : 0.0;
    mu = (float)mud;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
    if (blockIdx.y == 0 && tid < STRIP_CW && cc < C && running != nullptr) {   // torch BatchNorm1d buffers: momentum
      const double unb = M > 1 ? var * M / (M - 1) : var;                  // update with the unbiased variance
      running[cc] = (1.f - momentum) * running[cc] + momentum * mu;
      running[C + cc] = (1.f - momentum) * running[C + cc] + momentum * (float)unb;
    }
  } else if (cc < C) {
    mu = running[cc];
    rstd = 1.0f / sqrtf(running[C + cc] + eps);
  }
  if (tid < STRIP_CW && cc < C) {
    cf[0][c] = mu;
    cf[1][c] = rstd;
    cf[2][c] = gamma[cc];
    cf[3][c] = beta[cc];
    if (blockIdx.y == 0) {
      mean_rstd[2 * cc] = mu;
      mean_rstd[2 * cc + 1] = rstd;
    }
  }
  __syncthreads();
  const int cl = threadIdx.x * EPT, cg = blockIdx.x * STRIP_CW + cl;
  if (cg >= C) return;
  const int m0 = blockIdx.y * arows, m1 = min(M, m0 + arows);
  float mus[EPT], rs[EPT], ga[EPT], be[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) { mus[e] = cf[0][cl + e]; rs[e] = cf[1][cl + e]; ga[e] = cf[2][cl + e]; be[e] = cf[3][cl + e]; }
  for (int m = m0 + threadIdx.y; m < m1; m += UN * RL) {
    typename G::Vec v[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) v[u].load(a + (int64_t)min(m + u * RL, m1 - 1) * lda + cg);
#pragma unroll
    for (int u = 0; u < UN; ++u)
      if (m + u * RL < m1) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
          const float r = bn_act(v[u].v[e], act);
          v[u].v[e] = (r - mus[e]) * rs[e] * ga[e] + be[e];
        }
        v[u].store(y + (int64_t)(m + u * RL) * ldy + cg);
      }
  }
}
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const T* __restrict__ dy, int64_t lddy,
                                                             const T* __restrict__ dy2, int64_t lddy2,
                                                             const T* __restrict__ a, int64_t lda,
                                                             const float* __restrict__ mean_rstd,
                                                             float* __restrict__ partial, int M, int C, int act) {
  __shared__ float red[STRIP_RL_MAX][STRIP_CW][2];
  using G = StripGeom<T>;
  constexpr int EPT = G::EPT, RL = G::RL, UN = G::UN;
  const int cg = blockIdx.x * STRIP_CW + threadIdx.x * EPT;
  const int m0 = blockIdx.y * BN_PROWS, m1 = min(M, m0 + BN_PROWS);
  float s1[EPT] = {}, s2[EPT] = {};
  if (cg < C) {
    float mu[EPT], rs[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) { mu[e] = mean_rstd[2 * (cg + e)]; rs[e] = mean_rstd[2 * (cg + e) + 1]; }
    for (int m = m0 + threadIdx.y; m < m1; m += UN * RL) {
      typename G::Vec v[UN], d[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int64_t mm = min(m + u * RL, m1 - 1);
        v[u].load(a + mm * lda + cg);
        d[u].load(dy + mm * lddy + cg);
      }
      if (dy2 != nullptr) {                 // the gradient is dy + dy2 (two Res2Net branches), summed here
#pragma unroll
        for (int u = 0; u < UN; ++u) {
          typename G::Vec w;
          w.load(dy2 + (int64_t)min(m + u * RL, m1 - 1) * lddy2 + cg);
#pragma unroll
          for (int e = 0; e < EPT; ++e) d[u].v[e] += w.v[e];
        }
      }
#pragma unroll
      for (int u = 0; u < UN; ++u)
        if (m + u * RL < m1) {
#pragma unroll
          for (int e = 0; e < EPT; ++e) {
            const float r = bn_act(v[u].v[e], act);
            s1[e] += d[u].v[e];
            s2[e] = fmaf(d[u].v[e], (r - mu[e]) * rs[e], s2[e]);
          }
        }
    }
  }
  strip_store_partial2<EPT>(red, s1, s2, partial, (int64_t)blockIdx.y, C);
}
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dy, int64_t lddy,
                                                           const T* __restrict__ dy2, int64_t lddy2,
                                                           const T* __restrict__ a, int64_t lda,
                                                           const float* __restrict__ mean_rstd,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ partial, int nblk,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           T* __restrict__ da, int64_t ldda, int M, int C, int act,
                                                           float invM, float* __restrict__ cs_partial, int arows) {
  __shared__ double fold[4][STRIP_CW][2];
  __shared__ float csred[STRIP_RL_MAX][STRIP_CW];          // column sums of da over this workgroup's rows (cs_partial != NULL)
  __shared__ float cf[5][STRIP_CW];                 // mean, rstd, gamma*rstd, sum dy / M, sum dy xhat / M
  using G = StripGeom<T>;
  constexpr int EPT = G::EPT, RL = G::RL, UN = G::UN;
  const int tid = threadIdx.y * G::XL + threadIdx.x;
  const int c = tid & (STRIP_CW - 1), cc = blockIdx.x * STRIP_CW + c;
  double s1, s2;
  bn_fold(partial, nblk, C, fold, s1, s2, tid);
  if (tid < STRIP_CW && cc < C) {
    const float f1 = (float)s1, f2 = (float)s2, rstd = mean_rstd[2 * cc + 1];
    cf[0][c] = mean_rstd[2 * cc];
    cf[1][c] = rstd;
    cf[2][c] = gamma[cc] * rstd;
    cf[3][c] = f1 * invM;
    cf[4][c] = f2 * invM;
    if (blockIdx.y == 0) {                       // written, not accumulated
      dbeta[cc] = f1;
      dgamma[cc] = f2;
    }
  }
  __syncthreads();
  const int cl = threadIdx.x * EPT, cg = blockIdx.x * STRIP_CW + cl;
  if (cg >= C && cs_partial == nullptr) return;
  const int m0 = blockIdx.y * arows, m1 = (cg < C) ? min(M, m0 + arows) : m0;
  float mu[EPT], rs[EPT], gr[EPT], m1s[EPT], m2s[EPT], cs[EPT] = {};
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    mu[e] = cf[0][cl + e]; rs[e] = cf[1][cl + e]; gr[e] = cf[2][cl + e]; m1s[e] = cf[3][cl + e]; m2s[e] = cf[4][cl + e];
  }
  for (int m = m0 + threadIdx.y; m < m1; m += UN * RL) {
    typename G::Vec v[UN], d[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t mm = min(m + u * RL, m1 - 1);
      v[u].load(a + mm * lda + cg);
      d[u].load(dy + mm * lddy + cg);
    }
    if (dy2 != nullptr) {
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        typename G::Vec w;
        w.load(dy2 + (int64_t)min(m + u * RL, m1 - 1) * lddy2 + cg);
#pragma unroll
        for (int e = 0; e < EPT; ++e) d[u].v[e] += w.v[e];
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u)
      if (m + u * RL < m1) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
          const float av = v[u].v[e];
          const float r = bn_act(av, act);
          const float rh = (r - mu[e]) * rs[e];
          const float dr = gr[e] * (d[u].v[e] - m1s[e] - rh * m2s[e]);
          d[u].v[e] = (act && !(av > 0.f)) ? (act == BN_ACT_LEAKY ? BN_LEAKY_SLOPE * dr : 0.f) : dr;
          cs[e] += d[u].v[e];
        }
        d[u].store(da + (int64_t)(m + u * RL) * ldda + cg);
      }
  }
  // column sums of da (= the bias gradient of the convolution in front of this BatchNorm) while the values are in
  // registers: per row-block partials, folded by the caller (w2v2_colsum over nblk rows instead of M)
  // (the lane-order fold of strip_common.h spelled out: its shared forms flip the branch around this tail)
  if (cs_partial != nullptr) {
#pragma unroll
    for (int e = 0; e < EPT; ++e) csred[threadIdx.y][cl + e] = cs[e];
    __syncthreads();
    if (tid < STRIP_CW && cc < C) {
      float t = 0.f;
#pragma unroll
      for (int y = 0; y < RL; ++y) t += csred[y][c];
      cs_partial[(int64_t)blockIdx.y * C + cc] = t;
    }
  }
}

// ------------------------------------------------------------------------------------------ strided add
template <typename T>
__global__ void add_strided_kernel(const T* __restrict__ a, int64_t lda, const T* __restrict__ b, int64_t ldb,
                                   T* __restrict__ y, int64_t ldy, int M, int C) {
  constexpr int EPT = StripGeom<T>::EPT;
  const int nch = C / EPT;
  const int64_t total = (int64_t)M * nch;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % nch);
    const int64_t m = i / nch;
    typename StripGeom<T>::Vec va, vb;
    va.load(a + m * lda + ch * EPT);
    if (b != nullptr) {                    // b == NULL: a strided copy (Res2Net pass-through chunk, SE input slice)
      vb.load(b + m * ldb + ch * EPT);
#pragma unroll
      for (int e = 0; e < EPT; ++e) va.v[e] += vb.v[e];
    }
    va.store(y + m * ldy + ch * EPT);
  }
}

// ------------------------------------------------------------------------------------------ squeeze-excitation gate
// one 16-byte vector per thread (StripGeom: 8 channels of a 16-bit tensor, 4 of an f32 one); C % 8 == 0.
// y[b,t,c] = x[b,t,c] * g[b,c]
template <typename T>
__global__ void se_scale_kernel(const T* __restrict__ x, const float* __restrict__ g, T* __restrict__ y, int B, int Tn,
                                int C) {
  constexpr int EPT = StripGeom<T>::EPT;
  const int nch = C / EPT;
  const int total = B * Tn * nch;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int row = i / nch, ch = i - row * nch;
    const int b = row / Tn;
    typename StripGeom<T>::Vec v;
    typename StripGeom<T>::FVec gv;
    v.load(x + (int64_t)row * C + ch * EPT);
    gv.load(g + (int64_t)b * C + ch * EPT);
#pragma unroll
    for (int e = 0; e < EPT; ++e) v.v[e] *= gv.v[e];
    v.store(y + (int64_t)row * C + ch * EPT);
  }
}
// dg[b,c] = sum_t dout[b,t,c] * x[b,t,c]        blockDim = (StripGeom<T>::XL channel lanes, StripGeom<T>::RL time lanes)
template <typename T>
__global__ __launch_bounds__(256) void se_bwd_gate_kernel(const T* __restrict__ dout, const T* __restrict__ x,
                                                          float* __restrict__ dg, int Tn, int C) {
  __shared__ float red[STRIP_RL_MAX][STRIP_CW];
  constexpr int EPT = StripGeom<T>::EPT, XL = StripGeom<T>::XL, RL = StripGeom<T>::RL;
  const int b = blockIdx.y, cg = blockIdx.x * STRIP_CW + threadIdx.x * EPT;
  float s[EPT] = {};
  if (cg < C)
    for (int t = threadIdx.y; t < Tn; t += RL) {
      const int64_t i = ((int64_t)b * Tn + t) * C + cg;
      typename StripGeom<T>::Vec d, v;
      d.load(dout + i);
      v.load(x + i);
#pragma unroll
      for (int e = 0; e < EPT; ++e) s[e] = fmaf(d.v[e], v.v[e], s[e]);
    }
  // (strip_put / strip_lane_sum spelled out: every shared form re-schedules this tail, profiles/strip_pieces_device_code.txt)
#pragma unroll
  for (int e = 0; e < EPT; ++e) red[threadIdx.y][threadIdx.x * EPT + e] = s[e];
  __syncthreads();
  const int tid = threadIdx.y * XL + threadIdx.x;
  if (tid < STRIP_CW && blockIdx.x * STRIP_CW + tid < C) {
    float acc = 0.f;
#pragma unroll
    for (int yy = 0; yy < RL; ++yy) acc += red[yy][tid];
    dg[(int64_t)b * C + blockIdx.x * STRIP_CW + tid] = acc;
  }
}
// dx[b,t,c] = dout[b,t,c] * g[b,c] + ds[b,c] / T      (ds = gradient wrt the time mean that feeds the gate)
template <typename T>
__global__ void se_bwd_x_kernel(const T* __restrict__ dout, const float* __restrict__ g, const float* __restrict__ ds,
                                T* __restrict__ dx, int B, int Tn, int C) {
  constexpr int EPT = StripGeom<T>::EPT;
  const int nch = C / EPT;
  const int total = B * Tn * nch;
  const float invT = 1.0f / (float)Tn;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int row = i / nch, ch = i - row * nch;
    const int b = row / Tn;
    typename StripGeom<T>::Vec v;
    typename StripGeom<T>::FVec gv, sv;
    v.load(dout + (int64_t)row * C + ch * EPT);
    gv.load(g + (int64_t)b * C + ch * EPT);
    sv.load(ds + (int64_t)b * C + ch * EPT);
#pragma unroll
    for (int e = 0; e < EPT; ++e) v.v[e] = fmaf(v.v[e], gv.v[e], sv.v[e] * invT);
    v.store(dx + (int64_t)row * C + ch * EPT);
  }
}

// ------------------------------------------------------------------------------------------ statistics pooling (x-vector)
// speechbrain StatisticsPooling over time on an f32 channels-last [B][T][C] tensor with a row stride:
//   out[b] = cat(mean_t x, std_t x + eps)   (mean FIRST, unbiased std, eps added to the std -- the wav2vec2 pool of
//   pool.hip returns the std first and has no eps)
// Two passes in the torch.std_mean order: the mean, then the centred squares.  One workgroup per (128-channel strip,
// utterance): 32 channel lanes x 4 channels, 8 time lanes that walk the frames SP_UN at a time; the time lanes are folded
// through LDS in lane order -- a fixed order, no atomics, and the same order for an utterance of n frames whether it
// stands alone or in a padded batch (LEN: the first lens[b] frames of utterance b).  stats (may be NULL) keeps
// (mean, std) without the eps for the backward.
constexpr int SP_UN = 4;
template <bool LEN>
__global__ __launch_bounds__(256) void stat_pool_fwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                            float* __restrict__ out, float* __restrict__ stats,
                                                            const int* __restrict__ lens, int Tn, int C, float eps) {
  __shared__ float red[8][STRIP_CW];
  __shared__ float mean_s[STRIP_CW];
  using G = StripGeom<float>;
  constexpr int EPT = G::EPT, RL = G::RL;
  static_assert(RL == 8 && EPT == 4, "stat_pool: 32 channel lanes x 8 time lanes");
  const int b = blockIdx.y;
  const int tid = threadIdx.y * G::XL + threadIdx.x;
  const int cl = threadIdx.x * EPT, cg = blockIdx.x * STRIP_CW + cl;
  const int n = LEN ? lens[b] : Tn;
  const float* xb = x + (int64_t)b * Tn * ldx;
  const bool on = cg < C;
  float s[EPT] = {};
  if (on)
    for (int t = threadIdx.y; t < n; t += SP_UN * RL) {
      Vec4f v[SP_UN];
#pragma unroll
      for (int u = 0; u < SP_UN; ++u) v[u].load(xb + (int64_t)min(t + u * RL, n - 1) * ldx + cg);
#pragma unroll
      for (int u = 0; u < SP_UN; ++u)
        if (t + u * RL < n) {
#pragma unroll
          for (int e = 0; e < EPT; ++e) s[e] += v[u].v[e];
        }
    }
  strip_put<EPT>(red, s);
  if (tid < STRIP_CW) mean_s[tid] = strip_lane_sum<RL>(red, tid) / (float)n;
  __syncthreads();
  float mu[EPT], q[EPT] = {};
#pragma unroll
  for (int e = 0; e < EPT; ++e) mu[e] = mean_s[cl + e];
  if (on)
    for (int t = threadIdx.y; t < n; t += SP_UN * RL) {
      Vec4f v[SP_UN];
#pragma unroll
      for (int u = 0; u < SP_UN; ++u) v[u].load(xb + (int64_t)min(t + u * RL, n - 1) * ldx + cg);
#pragma unroll
      for (int u = 0; u < SP_UN; ++u)
        if (t + u * RL < n) {
#pragma unroll
          for (int e = 0; e < EPT; ++e) {
            const float d = v[u].v[e] - mu[e];
            q[e] = fmaf(d, d, q[e]);
          }
        }
    }
  strip_put<EPT>(red, q);
  const int cc = blockIdx.x * STRIP_CW + tid;
  if (tid < STRIP_CW && cc < C) {
    const float sd = sqrtf(strip_lane_sum<RL>(red, tid) / (float)(n - 1));
    const int64_t o = (int64_t)b * 2 * C;
    out[o + cc] = mean_s[tid];
    out[o + C + cc] = sd + eps;
    if (stats != nullptr) {
      stats[o + cc] = mean_s[tid];
      stats[o + C + cc] = sd;
    }
  }
}
// dx[b][t][c] = dmean[b][c] / T + dstd[b][c] (x - mean) / ((T - 1) std): one 16-byte vector per thread.  A constant
// column has std = 0, where the second term is 0 / 0: it is taken as 0, which is what torch's std backward returns there
// (it masks the division where the result is 0), so no NaN reaches the weights through the Linear's data gradient.
__global__ void stat_pool_bwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ stats,
                                     const float* __restrict__ dout, float* __restrict__ dx, int64_t lddx, int B, int Tn,
                                     int C) {
  const int cv = C >> 2;
  const int64_t total = (int64_t)B * Tn * cv;
  const float invT = 1.0f / (float)Tn, tm1 = (float)(Tn - 1);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / cv;
    const int c = (int)(i - row * cv) * 4;
    const int64_t o = (row / Tn) * 2 * C + c;
    Vec4f xv, mu, sd, dm, ds;
    xv.load(x + row * ldx + c);
    mu.load(stats + o);
    sd.load(stats + o + C);
    dm.load(dout + o);
    ds.load(dout + o + C);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      xv.v[e] = dm.v[e] * invT + (sd.v[e] > 0.f ? ds.v[e] * (xv.v[e] - mu.v[e]) / (tm1 * sd.v[e]) : 0.f);
    xv.store(dx + row * lddx + c);
  }
}

// ------------------------------------------------------------------------------------------ small f32 activations
// mode 0: relu, 1: sigmoid.  bwd takes the forward OUTPUT y.
__global__ void act_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int mode) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    y[i] = mode == 0 ? fmaxf(v, 0.f) : sigmoid_f(v);
  }
}
__global__ void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx,
                               int64_t n, int mode) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float yv = y[i];
    dx[i] = mode == 0 ? (yv > 0.f ? dy[i] : 0.f) : sigmoid_bwd_f(dy[i], yv);
  }
}

// ------------------------------------------------------------------------------------------ C ABI
extern "C" int w2v2_bn_workspace_floats(int M, int C) { return (int)cdiv(M, 128) * C * 2; }
// Rows per workgroup of the apply kernels: 256, or 64 where 256 would leave most CUs without a workgroup -- the 128-channel
// Res2Net slices of the ECAPA path are ONE strip wide: 78 workgroups of 256 rows at M = 19800 ran a 10 MB pass in 17-19 us
// (four dependent load rounds behind the statistics fold on 78 of 256 CUs), 310 workgroups of 64 rows do one round each.
static int bn_arows(int M, int C) { return cdiv(C, STRIP_CW) * cdiv(M, BN_AROWS) >= 256 ? BN_AROWS : 64; }
extern "C" int w2v2_bn_colsum_rows(int M, int C) { return (int)cdiv(M, bn_arows(M, C)); }

// One thread owns one 16-byte vector of a row (StripGeom): 8 channels of a 16-bit tensor, 4 of an f32 one, and every guard of
// the strip kernels is per vector -- so C and the row strides are multiples of 8, or of 4 for f32 (the x-vector's last
// TDNN layer has 1500 channels: 1500 % 8 = 4).  The partial-sum fold reads channel PAIRS, which any such C keeps whole.
static int bn_align(int dtype) { return dtype == W2V2_F32 ? 4 : 8; }
extern "C" int w2v2_bn_fwd(const void* a, int64_t lda, float* workspace, float* mean_rstd, float* running,
                           const float* gamma, const float* beta, void* y, int64_t ldy, int M, int C, float eps,
                           float momentum, int act, int train, int dtype, void* stream) {
  const int al = bn_align(dtype);
  W2V2_REQUIRE(a && mean_rstd && gamma && beta && y && M > 0 && C > 0 && C % al == 0 && lda >= C && lda % al == 0 &&
                   ldy % al == 0 && act >= 0 && act <= BN_ACT_LEAKY,
               "bn_fwd: bad arguments (C, lda, ldy multiples of 8, of 4 for f32; act 0, 1 or 2)");
  W2V2_REQUIRE(train ? workspace != nullptr : running != nullptr,
               "bn_fwd: training needs the workspace, evaluation the running statistics");
  const int nblk = (int)cdiv(M, BN_PROWS);
  const int arows = bn_arows(M, C);
  const dim3 gp((unsigned)cdiv(C, STRIP_CW), nblk), ga((unsigned)cdiv(C, STRIP_CW), (unsigned)cdiv(M, arows));
  hipStream_t st = as_stream(stream);
#define TD_BNF(T_)                                                                                                   \
  if (train)                                                                                                         \
    hipLaunchKernelGGL(bn_partial_kernel<T_>, gp, dim3(StripGeom<T_>::XL, StripGeom<T_>::RL), 0, st, (const T_*)a, lda, workspace, M, C, act);             \
  hipLaunchKernelGGL(bn_apply_kernel<T_>, ga, dim3(StripGeom<T_>::XL, StripGeom<T_>::RL), 0, st, (const T_*)a, lda, workspace, nblk, mean_rstd, running,    \
                     gamma, beta, (T_*)y, ldy, M, C, act, eps, momentum, train, arows)
  W2V2_DISPATCH_ACT(dtype, "bn_fwd", TD_BNF(AT););
#undef TD_BNF
  W2V2_CHECK_LAUNCH("bn_fwd");
  return 0;
}

static int bn_bwd_impl(const void* dy, int64_t lddy, const void* dy2, int64_t lddy2, const void* a, int64_t lda,
                       const float* mean_rstd, const float* gamma, float* workspace, float* dgamma, float* dbeta, void* da,
                       int64_t ldda, int M, int C, int act, float* colsum_partial, int dtype, void* stream) {
  const int al = bn_align(dtype);
  W2V2_REQUIRE(dy && a && mean_rstd && gamma && workspace && dgamma && dbeta && da && M > 0 && C > 0 && C % al == 0 &&
                   lda % al == 0 && lddy % al == 0 && ldda % al == 0 && (dy2 == nullptr || lddy2 % al == 0) && act >= 0 &&
                   act <= BN_ACT_LEAKY,
               "bn_bwd: bad arguments (C and strides multiples of 8, of 4 for f32; act 0, 1 or 2)");
  const int nblk = (int)cdiv(M, BN_PROWS);
  const int arows = bn_arows(M, C);
  const dim3 gp((unsigned)cdiv(C, STRIP_CW), nblk), ga((unsigned)cdiv(C, STRIP_CW), (unsigned)cdiv(M, arows));
  hipStream_t st = as_stream(stream);
#define TD_BNB(T_)                                                                                                  \
  hipLaunchKernelGGL(bn_bwd_partial_kernel<T_>, gp, dim3(StripGeom<T_>::XL, StripGeom<T_>::RL), 0, st, (const T_*)dy, lddy, (const T_*)dy2, lddy2,         \
                     (const T_*)a, lda, mean_rstd, workspace, M, C, act);                                          \
  hipLaunchKernelGGL(bn_bwd_apply_kernel<T_>, ga, dim3(StripGeom<T_>::XL, StripGeom<T_>::RL), 0, st, (const T_*)dy, lddy, (const T_*)dy2, lddy2,           \
                     (const T_*)a, lda, mean_rstd, gamma, workspace, nblk, dgamma, dbeta, (T_*)da, ldda, M, C, act, \
                     1.0f / (float)M, colsum_partial, arows)
  W2V2_DISPATCH_ACT(dtype, "bn_bwd", TD_BNB(AT););
#undef TD_BNB
  W2V2_CHECK_LAUNCH("bn_bwd");
  return 0;
}
extern "C" int w2v2_bn_bwd(const void* dy, int64_t lddy, const void* a, int64_t lda, const float* mean_rstd,
                           const float* gamma, float* workspace, float* dgamma, float* dbeta, void* da, int64_t ldda,
                           int M, int C, int act, float* colsum_partial, int dtype, void* stream) {
  return bn_bwd_impl(dy, lddy, nullptr, 0, a, lda, mean_rstd, gamma, workspace, dgamma, dbeta, da, ldda, M, C, act,
                     colsum_partial, dtype, stream);
}
// the same with the output gradient given as dy + dy2 (two row-strided operands of one shape; both kernels add them as
// they read): the Res2Net chunk whose output feeds the next chunk AND the block's concatenation
extern "C" int w2v2_bn_bwd_sum(const void* dy, int64_t lddy, const void* dy2, int64_t lddy2, const void* a, int64_t lda,
                               const float* mean_rstd, const float* gamma, float* workspace, float* dgamma, float* dbeta,
                               void* da, int64_t ldda, int M, int C, int act, float* colsum_partial, int dtype,
                               void* stream) {
  W2V2_REQUIRE(dy2 != nullptr, "bn_bwd_sum: null second operand");
  return bn_bwd_impl(dy, lddy, dy2, lddy2, a, lda, mean_rstd, gamma, workspace, dgamma, dbeta, da, ldda, M, C, act,
                     colsum_partial, dtype, stream);
}

// lens: device int32 [B] for the variable-length form (dilation * (k - 1) / 2 < lens[b] <= T, checked by the caller on
// the host), null for fixed length
static int im2col_reflect_impl(const char* name, const void* x, int64_t ldx, const void* x2, int64_t ldx2, void* col,
                               const int* lens, int B, int T, int Cin, int k, int dilation, int dtype, void* stream) {
  W2V2_REQUIRE(x && col && B > 0 && T > 0 && Cin % 8 == 0 && k % 2 == 1 && dilation >= 1 && ldx % 8 == 0 &&
                   (x2 == nullptr || ldx2 % 8 == 0) && dilation * (k - 1) / 2 < T,
               "%s: bad arguments (odd k, Cin %% 8 == 0, padding < T)", name);
  const TapGeom g{B, T, T, Cin, k, 1, dilation, (k - 1) / 2 * dilation};
  W2V2_DISPATCH_LEN(lens, W2V2_DISPATCH_ACT(dtype, name,
    return (tap_gather_launch<AT, PadReflect, LEN>(name, (const AT*)x, ldx, (const AT*)x2, ldx2, (AT*)col, lens, g, stream));));
}
extern "C" int w2v2_im2col_reflect(const void* x, int64_t ldx, void* col, int B, int T, int Cin, int k, int dilation,
                                   int dtype, void* stream) {
  return im2col_reflect_impl("im2col_reflect", x, ldx, nullptr, 0, col, nullptr, B, T, Cin, k, dilation, dtype, stream);
}
// the taps of x + x2 (same shape, own row strides): the Res2Net chunk input x_i + y_{i-1} without materialising the sum
extern "C" int w2v2_im2col_reflect_sum(const void* x, int64_t ldx, const void* x2, int64_t ldx2, void* col, int B, int T,
                                       int Cin, int k, int dilation, int dtype, void* stream) {
  W2V2_REQUIRE(x2 != nullptr, "im2col_reflect_sum: null second operand");
  return im2col_reflect_impl("im2col_reflect", x, ldx, x2, ldx2, col, nullptr, B, T, Cin, k, dilation, dtype, stream);
}
extern "C" int w2v2_im2col_reflect_len(const void* x, int64_t ldx, void* col, const int* lens, int B, int T, int Cin,
                                       int k, int dilation, int dtype, void* stream) {
  W2V2_REQUIRE(lens != nullptr, "im2col_reflect_len: bad arguments (null lens)");
  return im2col_reflect_impl("im2col_reflect_len", x, ldx, nullptr, 0, col, lens, B, T, Cin, k, dilation, dtype, stream);
}
extern "C" int w2v2_im2col_reflect_sum_len(const void* x, int64_t ldx, const void* x2, int64_t ldx2, void* col,
                                           const int* lens, int B, int T, int Cin, int k, int dilation, int dtype,
                                           void* stream) {
  W2V2_REQUIRE(x2 != nullptr, "im2col_reflect_sum_len: null second operand");
  W2V2_REQUIRE(lens != nullptr, "im2col_reflect_len: bad arguments (null lens)");
  return im2col_reflect_impl("im2col_reflect_len", x, ldx, x2, ldx2, col, lens, B, T, Cin, k, dilation, dtype, stream);
}

extern "C" int w2v2_col2im_reflect(const void* dcol, void* dx, int64_t lddx, int B, int T, int Cin, int k, int dilation,
                                   int accumulate, int dtype, void* stream) {
  W2V2_REQUIRE(dcol && dx && B > 0 && T > 0 && Cin % 8 == 0 && k % 2 == 1 && dilation >= 1 && lddx % 8 == 0 &&
                   dilation * (k - 1) / 2 < T,
               "col2im_reflect: bad arguments");
  const TapGeom g{B, T, T, Cin, k, 1, dilation, (k - 1) / 2 * dilation};
  W2V2_DISPATCH_ACT(dtype, "col2im_reflect",
    return (tap_adjoint_launch<AT, PadReflect, true>("col2im_reflect", (const AT*)dcol, (AT*)dx, lddx, g, accumulate, stream)););
}

extern "C" int w2v2_add_strided(const void* a, int64_t lda, const void* b, int64_t ldb, void* y, int64_t ldy, int M,
                                int C, int dtype, void* stream) {
  W2V2_REQUIRE(a && y && M > 0 && C % 8 == 0 && lda % 8 == 0 && (b == nullptr || ldb % 8 == 0) && ldy % 8 == 0,
               "add_strided: bad arguments");
  const int nb = blocks256((int64_t)M * (C / bn_align(dtype)));
  hipStream_t st = as_stream(stream);
  W2V2_DISPATCH_ACT(dtype, "add_strided",
    hipLaunchKernelGGL(add_strided_kernel<AT>, dim3(nb), dim3(256), 0, st, (const AT*)a, lda,
                           (const AT*)b, ldb, (AT*)y, ldy, M, C););
  W2V2_CHECK_LAUNCH("add_strided");
  return 0;
}

extern "C" int w2v2_se_scale(const void* x, const float* g, void* y, int B, int T, int C, int dtype, void* stream) {
  W2V2_REQUIRE(x && g && y && B > 0 && T > 0 && C > 0 && C % 8 == 0, "se_scale: bad arguments (C %% 8 == 0)");
  const int nb = blocks256((int64_t)B * T * (C / bn_align(dtype)));
  hipStream_t st = as_stream(stream);
  W2V2_DISPATCH_ACT(dtype, "se_scale",
    hipLaunchKernelGGL(se_scale_kernel<AT>, dim3(nb), dim3(256), 0, st, (const AT*)x, g, (AT*)y, B, T, C););
  W2V2_CHECK_LAUNCH("se_scale");
  return 0;
}

extern "C" int w2v2_se_bwd_gate(const void* dout, const void* x, float* dg, int B, int T, int C, int dtype,
                                void* stream) {
  W2V2_REQUIRE(dout && x && dg && B > 0 && T > 0 && C > 0 && C % 8 == 0, "se_bwd_gate: bad arguments (C %% 8 == 0)");
  dim3 grid((unsigned)cdiv(C, STRIP_CW), B);
  hipStream_t st = as_stream(stream);
  W2V2_DISPATCH_ACT(dtype, "se_bwd_gate",
    hipLaunchKernelGGL(se_bwd_gate_kernel<AT>, grid, dim3(StripGeom<AT>::XL, StripGeom<AT>::RL), 0, st, (const AT*)dout, (const AT*)x, dg, T, C););
  W2V2_CHECK_LAUNCH("se_bwd_gate");
  return 0;
}

extern "C" int w2v2_se_bwd_x(const void* dout, const float* g, const float* ds, void* dx, int B, int T, int C, int dtype,
                             void* stream) {
  W2V2_REQUIRE(dout && g && ds && dx && B > 0 && T > 0 && C > 0 && C % 8 == 0, "se_bwd_x: bad arguments (C %% 8 == 0)");
  const int nb = blocks256((int64_t)B * T * (C / bn_align(dtype)));
  hipStream_t st = as_stream(stream);
  W2V2_DISPATCH_ACT(dtype, "se_bwd_x",
    hipLaunchKernelGGL(se_bwd_x_kernel<AT>, dim3(nb), dim3(256), 0, st, (const AT*)dout, g, ds, (AT*)dx,
                           B, T, C););
  W2V2_CHECK_LAUNCH("se_bwd_x");
  return 0;
}

extern "C" int w2v2_act_fwd(const float* x, float* y, int64_t n, int mode, void* stream) {
  W2V2_REQUIRE(x && y && n > 0 && (mode == 0 || mode == 1), "act_fwd: bad arguments");
  hipLaunchKernelGGL(act_fwd_kernel, dim3(blocks256(n)), dim3(256), 0, as_stream(stream), x, y, n, mode);
  W2V2_CHECK_LAUNCH("act_fwd");
  return 0;
}

extern "C" int w2v2_act_bwd(const float* dy, const float* y, float* dx, int64_t n, int mode, void* stream) {
  W2V2_REQUIRE(dy && y && dx && n > 0 && (mode == 0 || mode == 1), "act_bwd: bad arguments");
  hipLaunchKernelGGL(act_bwd_kernel, dim3(blocks256(n)), dim3(256), 0, as_stream(stream), dy, y, dx, n, mode);
  W2V2_CHECK_LAUNCH("act_bwd");
  return 0;
}

// x f32 [B][T] rows of C channels with row stride ldx; out / stats / dout f32 [B][2C]; lens (the _len form): device int32 [B],
// 2 <= lens[b] <= T (checked by the caller on the host)
static int stat_pool_fwd_impl(const char* name, const float* x, int64_t ldx, float* out, float* stats, const int* lens,
                              int B, int T, int C, float eps, void* stream) {
  W2V2_REQUIRE(x && out && B > 0 && T >= 2 && C > 0 && C % 4 == 0 && ldx >= C && ldx % 4 == 0 &&
                   (reinterpret_cast<uintptr_t>(x) & 15) == 0,
               "%s: bad arguments (T >= 2, C and ldx multiples of 4, 16-byte aligned x)", name);
  const dim3 grid((unsigned)cdiv(C, STRIP_CW), (unsigned)B), block(StripGeom<float>::XL, StripGeom<float>::RL);
  hipStream_t st = as_stream(stream);
  W2V2_DISPATCH_LEN(lens, hipLaunchKernelGGL(stat_pool_fwd_kernel<LEN>, grid, block, 0, st, x, ldx, out, stats, lens, T, C, eps));
  W2V2_CHECK_LAUNCH(name);
  return 0;
}
extern "C" int w2v2_stat_pool_fwd(const float* x, int64_t ldx, float* out, float* stats, int B, int T, int C, float eps,
                                  void* stream) {
  return stat_pool_fwd_impl("stat_pool_fwd", x, ldx, out, stats, nullptr, B, T, C, eps, stream);
}
extern "C" int w2v2_stat_pool_fwd_len(const float* x, int64_t ldx, float* out, float* stats, const int* lens, int B, int T,
                                      int C, float eps, void* stream) {
  W2V2_REQUIRE(lens != nullptr, "stat_pool_fwd_len: bad arguments (null lens)");
  return stat_pool_fwd_impl("stat_pool_fwd_len", x, ldx, out, stats, lens, B, T, C, eps, stream);
}
extern "C" int w2v2_stat_pool_bwd(const float* x, int64_t ldx, const float* stats, const float* dout, float* dx,
                                  int64_t lddx, int B, int T, int C, void* stream) {
  W2V2_REQUIRE(x && stats && dout && dx && B > 0 && T >= 2 && C > 0 && C % 4 == 0 && ldx >= C && ldx % 4 == 0 &&
                   lddx >= C && lddx % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dx)) & 15) == 0,
               "stat_pool_bwd: bad arguments (T >= 2, C and strides multiples of 4, 16-byte aligned x and dx)");
  hipLaunchKernelGGL(stat_pool_bwd_kernel, dim3(blocks256((int64_t)B * T * (C >> 2))), dim3(256), 0, as_stream(stream), x,
                     ldx, stats, dout, dx, lddx, B, T, C);
  W2V2_CHECK_LAUNCH("stat_pool_bwd");
  return 0;
}
