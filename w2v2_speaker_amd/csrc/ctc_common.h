// ctc_common.h -- the device pieces that ctc.hip (one wavefront per utterance, at most 31 labels) and ctc_long.hip (one
// workgroup per utterance, at most 1023 labels) share: the (mantissa, int exponent) arithmetic of the recursion, the
// exponential with denormal results, the test of the length pair, the class of an extended state, the row pass of
// one frame, the state posterior and the 4-wide gradient store.  See the head of ctc.hip for why the recursion runs on probabilities.
#pragma once
#include "common.h"

constexpr int CTC_ZERO_E = -(1 << 28);    // exponent of the value 0 (m = 0)
// (256 threads, one row per workgroup: the row passes run on B * T = 9834 workgroups, enough to fill the chip with six
//  16-byte loads per thread and pass; aam_row_kernel needs 1024 threads because it has B = 66 workgroups in all)
constexpr int CTC_ROW_THREADS = 256;

struct CtcME { float m; int e; };        // m * 2^e, m >= 0
__device__ __forceinline__ CtcME ctc_zero() { return CtcME{0.f, CTC_ZERO_E}; }
__device__ __forceinline__ CtcME ctc_norm(float v, int e) {
  if (!(v > 0.f)) return ctc_zero();
  int k;
  const float m = frexpf(v, &k);
  return CtcME{m, e + k};
}
// a + b + c in this order, at the largest exponent of the three (not normalised)
__device__ __forceinline__ CtcME ctc_sum3(CtcME a, CtcME b, CtcME c) {
  const int em = max(a.e, max(b.e, c.e));
  const float v = ldexpf(a.m, max(a.e - em, -200)) + ldexpf(b.m, max(b.e - em, -200)) + ldexpf(c.m, max(c.e - em, -200));
  return CtcME{v, em};
}

// exp(x), x <= 0, with a correctly rounded DENORMAL result where the value is one (the hardware exponential flushes them):
// under the reference's blank bias every off-blank softmax entry of a frame is e^-100 = 3.7e-44, and for an utterance
// with an empty target those entries are the whole gradient
__device__ __forceinline__ float ctc_exp(float x) {
  const float y = x * 1.44269504088896341f;
  if (!(y > -151.f)) return 0.f;
  const float fl = floorf(y);
  return ldexpf(__builtin_amdgcn_exp2f(y - fl), (int)fl);
}

// Is the length pair of utterance b usable?  (input length in [0, T], target length in [0, W])
__device__ __forceinline__ bool ctc_bad_lengths(int Tb, int L, int T, int W) { return Tb < 0 || Tb > T || L < 0 || L > W; }
// class of extended state s (odd s: target (s - 1) / 2 + offset); sets bad when it is outside [0, C) or the blank
__device__ __forceinline__ int ctc_state_class(const int64_t* __restrict__ trow, int s, int S, int toff, int blank, int C,
                                               bool& bad) {
  bad = false;
  if (!(s & 1) || s >= S) return blank;
  const int64_t tv = trow[s >> 1] + toff;
  bad = tv < 0 || tv >= C || tv == blank;
  return bad ? blank : (int)tv;
}

// The row pass of one frame by a workgroup of CTC_ROW_THREADS threads: row maximum, 1 / sum exp, off-blank softmax mass
// and the L + 1 emission probabilities the frame's lattice column needs (blank + the utterance's targets).  WIDE = false:
// L + 1 <= 32 slots, one thread each (ctc.hip); WIDE = true: any L, the targets checked and the slots filled in loops over
// the workgroup (ctc_long.hip).  rowstat [rows] {row max, 1 / sum exp, off-blank mass, -}; pm / pe [rows][W + 1].
template <bool WIDE>
__device__ __forceinline__ void ctc_row_pass(const float* __restrict__ logits, int64_t ldc, const int64_t* __restrict__ targets,
                                             int64_t tstride, int W, int toff, const int* __restrict__ in_len,
                                             const int* __restrict__ tgt_len, int blank, float4* __restrict__ rowstat,
                                             float* __restrict__ pm, int* __restrict__ pe, int T, int C) {
  constexpr int NT = CTC_ROW_THREADS, NW = NT / 64;
  __shared__ float sh[NW], sh2[NW];
  const int64_t r = blockIdx.x;
  const int b = (int)(r / T), t = (int)(r - (int64_t)b * T), tid = threadIdx.x;
  const int Tb = in_len[b], L = tgt_len[b];
  // (block-uniform) a bad row or a frame past the utterance's end: the lattice never reads it, nothing is read here
  if (ctc_bad_lengths(Tb, L, T, W) || t >= Tb) return;
  bool badt = false;
  int cls = 0;
  if constexpr (WIDE) {
    for (int l = tid; l < L; l += NT) {
      bool bd;
      ctc_state_class(targets + (int64_t)b * tstride, 2 * l + 1, 2 * L + 1, toff, blank, C, bd);
      badt = badt || bd;
    }
  } else {
    if (tid <= L) cls = ctc_state_class(targets + (int64_t)b * tstride, tid == 0 ? 0 : 2 * tid - 1, 2 * L + 1, toff, blank, C, badt);
  }
  if (__syncthreads_or(badt)) return;
  const float* zr = logits + r * ldc;
  const bool vec = (ldc & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
  const float4* z4 = reinterpret_cast<const float4*>(zr);
  const int nv = (C + 3) >> 2;            // (ldc % 4 == 0: the last vector ends inside the row's padding, masked below)
  // Maximum and sum over the classes OFF the blank; the blank joins as a scalar.  Under the reference's blank bias the
  // off-blank mass is e^-100 of the row: summed against the row maximum it would be a sum of denormals (or of zeros),
  // summed against its own maximum it keeps f32's relative precision and is scaled once.
  float mxo = -INFINITY;
  if (vec) {
    for (int v = tid; v < nv; v += NT) {
      const float4 q = z4[v];
      const float z[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * v + i < C && 4 * v + i != blank) mxo = fmaxf(mxo, z[i]);
    }
  } else {
    for (int c = tid; c < C; c += NT)
      if (c != blank) mxo = fmaxf(mxo, zr[c]);
  }
  mxo = block_reduce_n<NW>(mxo, sh, true);
  float so = 0.f;
  if (vec) {
    for (int v = tid; v < nv; v += NT) {
      const float4 q = z4[v];
      const float z[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * v + i < C && 4 * v + i != blank) so += __expf(z[i] - mxo);
    }
  } else {
    for (int c = tid; c < C; c += NT)
      if (c != blank) so += __expf(zr[c] - mxo);
  }
  so = block_reduce_n<NW>(so, sh2, false);
  const float zb = zr[blank], mx = fmaxf(mxo, zb);
  const float sum_off = so * ctc_exp(mxo - mx), sum = sum_off + ctc_exp(zb - mx);
  const float inv = 1.0f / sum;
  // the off-blank softmax mass: where softmax[blank] > 1/2 the blank gradient is formed from it and the label
  // posteriors, two small sums (the gradient kernels), like p_y - 1 in aam_row_kernel
  if (tid == 0) rowstat[r] = make_float4(mx, inv, sum_off * inv, 0.f);
  for (int k = tid; k <= L; k += NT) {         // (WIDE = false: L + 1 <= NT, one trip)
    if constexpr (WIDE) cls = k == 0 ? blank : (int)(targets[(int64_t)b * tstride + k - 1] + toff);
    // log p = (z - max) - log(sum): the difference in double, so that the emission of a class 100 below the maximum (the
    // reference's blank bias) keeps f32's relative precision; log(sum) is common to the frame and cancels in the posteriors
    const double x = (((double)zr[cls] - (double)mx) - (double)logf(sum)) * 1.4426950408889634;
    float m = 0.f;
    int e = CTC_ZERO_E;
    if (x > -1.0e8) {
      const double fl = floor(x);
      m = exp2f((float)(x - fl));
      e = (int)fl;
    }
    pm[r * (W + 1) + k] = m;
    pe[r * (W + 1) + k] = e;
    if constexpr (!WIDE) break;
  }
}

// the state posterior alpha_t(s) beta~_t(s) / P from its three (m, e) pairs
__device__ __forceinline__ float ctc_posterior(float am, int ae, float bm, int be, float pm, int pe) {
  if (!(am > 0.f && bm > 0.f)) return 0.f;
  return ldexpf(am * bm / pm, min(max(ae + be - pe, -300), 300));
}

template <typename TG>
__device__ __forceinline__ void ctc_store4(TG* p, const float* g) {
  if constexpr (sizeof(TG) == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(g[0], g[1], g[2], g[3]);
  } else {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack2<TG>(g[0], g[1]), pack2<TG>(g[2], g[3]));
  }
}
