// ctc.hip -- CTC loss on the device (ref: src/optim/loss/ctc_loss.py:36-58 -> F.ctc_loss(log_softmax(logits), blank,
// reduction="mean", zero_infinity=True); speaker path: src/lightning_modules/speaker/speaker_recognition_module.py:222-244).
// The reference copies the [T, B, C] log-probabilities to the host and runs torch's CPU kernel; here nothing leaves the
// device.  Three launches over logits [B*T][ldc] f32 (utterance-major rows, like the no-pooling CE head's):
//   ctc_row_kernel      row maximum, 1 / sum exp, off-blank softmax mass and the L + 1 emission probabilities a frame's
//                       lattice column needs (blank + the utterance's targets)
//   ctc_lattice_kernel  one wavefront per utterance, extended state s = lane (2L + 1 <= 63 states): alpha forward over t,
//                       beta backward, the loss row
//   ctc_grad_kernel     state posteriors gamma_t(s) = alpha_t(s) beta~_t(s) / P, merged per class, and the dense row
//                       dlogit[t][c] = (softmax_t[c] - sum_{s: class(s) = c} gamma_t(s)) * scale / (B * max(L, 1))
// Arithmetic of the recursion: every quantity is a PROBABILITY kept as (mantissa, exponent) = m * 2^e with an int exponent
// per lane.  Sums of positive terms and products keep f32's RELATIVE precision (6e-8 per operation) whatever the
// magnitude, there is no transcendental in the recursion, and nothing under- or overflows: log-domain f32 (torch's own
// F.ctc_loss) carries an ABSOLUTE rounding error of ulp(|log alpha|), 1e-4 at the |log alpha| ~ 1.4e3 of a 149-frame
// utterance over 5995 classes, which is a relative error of the posterior.  beta~_t(s) leaves out the emission at t
// (alpha_t has it), so no posterior is divided by an emission probability.
#include "ctc_common.h"

constexpr int CTC_MAX_L = 31;             // 2L + 1 <= 63 states: the lattice column of one utterance is one wavefront
constexpr int CTC_STAGE = 4096;           // emission slots staged in LDS per chunk of frames (2 x 16 KiB)

// the caller's workspace, cut up (everything 4-byte elements; rowstat 16-byte, alpha / beta 8-byte aligned)
struct CtcWs {
  float4* info;      // [B]     {P mantissa, P exponent (int bits), status: 0 ok / 1 infeasible / 2 bad row, -}
  float4* rowstat;   // [rows]  {row max, 1 / sum exp, off-blank softmax mass, -}
  float* pm;         // [rows][W + 1]   emission probability of slot k (0 = blank, k = target k - 1): mantissa in [1, 2)
  int* pe;           //                 ... and exponent
  float2* alpha;     // [rows][2W + 1]  {m, e (int bits)} with the emission at t
  float2* beta;      // [rows][2W + 1]  ... without it
};
static __host__ __device__ inline int64_t ctc_ws_floats(int B, int64_t rows, int W) {
  return 4 * (int64_t)B + rows * (4 + 2 * (W + 1) + 4 * (2 * W + 1));
}
static inline CtcWs ctc_carve(float* ws, int B, int64_t rows, int W) {
  CtcWs w;
  float* p = ws;
  w.info = reinterpret_cast<float4*>(p); p += 4 * (int64_t)B;
  w.rowstat = reinterpret_cast<float4*>(p); p += 4 * rows;
  w.pm = p; p += rows * (W + 1);
  w.pe = reinterpret_cast<int*>(p); p += rows * (W + 1);
  w.alpha = reinterpret_cast<float2*>(p); p += 2 * rows * (2 * W + 1);
  w.beta = reinterpret_cast<float2*>(p);
  return w;
}

__device__ __forceinline__ CtcME ctc_lane(CtcME v, int src) {        // the value of lane `src` (out of range: zero)
  const float m = __shfl(v.m, src & 63, 64);
  const int e = __shfl(v.e, src & 63, 64);
  return (src < 0 || src > 63) ? ctc_zero() : CtcME{m, e};
}

__global__ __launch_bounds__(CTC_ROW_THREADS) void ctc_row_kernel(const float* __restrict__ logits, int64_t ldc,
                                                                  const int64_t* __restrict__ targets, int64_t tstride, int W,
                                                                  int toff, const int* __restrict__ in_len,
                                                                  const int* __restrict__ tgt_len, int blank, CtcWs ws, int T,
                                                                  int C) {
  ctc_row_pass<false>(logits, ldc, targets, tstride, W, toff, in_len, tgt_len, blank, ws.rowstat, ws.pm, ws.pe, T, C);
}

__global__ __launch_bounds__(64) void ctc_lattice_kernel(const int64_t* __restrict__ targets, int64_t tstride, int W, int toff,
                                                         const int* __restrict__ in_len, const int* __restrict__ tgt_len,
                                                         int blank, CtcWs ws, float* __restrict__ loss_rows, int T, int C) {
  __shared__ float pm_s[CTC_STAGE];
  __shared__ int pe_s[CTC_STAGE];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = in_len[b], L = tgt_len[b];
  bool bad = ctc_bad_lengths(Tb, L, T, W), badt = false;
  const int S = bad ? 1 : 2 * L + 1;
  const int cls = ctc_state_class(targets + (int64_t)b * tstride, lane, S, toff, blank, C, badt);
  bad = bad || __ballot(badt) != 0ull;
  if (bad) {                                   // NaN loss row, zero gradient (the bad_label convention of aam_row_kernel)
    if (lane == 0) {
      loss_rows[b] = __builtin_nanf("");
      ws.info[b] = make_float4(0.f, 0.f, 2.f, 0.f);
    }
    return;
  }
  const int W1 = W + 1, SP = 2 * W + 1;
  const int cls_m2 = __shfl(cls, (lane + 62) & 63, 64), cls_p2 = __shfl(cls, (lane + 2) & 63, 64);
  const bool live = lane < S;
  const bool skip_to = (lane & 1) && lane >= 3 && live && cls != cls_m2;        // s - 2 -> s (different labels only)
  const bool skip_from = (lane & 1) && lane + 2 < S && cls_p2 != cls;          // s -> s + 2
  const int slot = (lane & 1) ? (lane + 1) >> 1 : 0;
  const int64_t row0 = (int64_t)b * T;
  const int nfmax = CTC_STAGE / W1;
  // alpha: the virtual column before frame 0 holds 1 in state 0, so frame 0 needs no case of its own
  CtcME at = lane == 0 ? CtcME{0.5f, 1} : ctc_zero();
  for (int t0 = 0; t0 < Tb; t0 += nfmax) {
    const int nf = min(nfmax, Tb - t0);
    __syncthreads();
    for (int i = lane; i < nf * W1; i += 64) {
      pm_s[i] = ws.pm[(row0 + t0) * W1 + i];
      pe_s[i] = ws.pe[(row0 + t0) * W1 + i];
    }
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
      const CtcME p1 = ctc_lane(at, lane - 1), p2 = ctc_lane(at, lane - 2);
      const CtcME v = ctc_sum3(at, p1, skip_to ? p2 : ctc_zero());
      at = live ? ctc_norm(v.m * pm_s[f * W1 + slot], v.e + pe_s[f * W1 + slot]) : ctc_zero();
      if (lane < SP) ws.alpha[(row0 + t0 + f) * SP + lane] = make_float2(at.m, __int_as_float(at.e));
    }
  }
  // P = alpha_{Tb-1}(S - 1) + alpha_{Tb-1}(S - 2)
  const CtcME pv = ctc_sum3(ctc_lane(at, S - 1), ctc_lane(at, S - 2), ctc_zero());
  const CtcME P = ctc_norm(pv.m, pv.e);
  if (lane == 0) {
    // zero_infinity: an infeasible utterance (P = 0) contributes 0 to the loss and to the gradient
    const bool feasible = P.m > 0.f;
    loss_rows[b] = feasible ? -fmaf((float)P.e, 0.69314718055994531f, logf(P.m)) / (float)max(L, 1) : 0.f;
    ws.info[b] = make_float4(P.m, __int_as_float(P.e), feasible ? 0.f : 1.f, 0.f);
  }
  if (!(P.m > 0.f)) return;
  // beta~_t(s): everything after frame t, WITHOUT the emission at t; beta~_{Tb-1} = 1 in the two final states
  CtcME bt = (lane == S - 1 || lane == S - 2) ? CtcME{0.5f, 1} : ctc_zero();
  const int nchunk = (Tb + nfmax - 1) / nfmax;
  for (int ch = nchunk - 1; ch >= 0; --ch) {
    const int t0 = ch * nfmax, nf = min(nfmax, Tb - t0);
    __syncthreads();
    for (int i = lane; i < nf * W1; i += 64) {
      pm_s[i] = ws.pm[(row0 + t0) * W1 + i];
      pe_s[i] = ws.pe[(row0 + t0) * W1 + i];
    }
    __syncthreads();
    for (int f = nf - 1; f >= 0; --f) {
      if (lane < SP) ws.beta[(row0 + t0 + f) * SP + lane] = make_float2(bt.m, __int_as_float(bt.e));
      const CtcME full = live ? CtcME{bt.m * pm_s[f * W1 + slot], bt.m > 0.f ? bt.e + pe_s[f * W1 + slot] : CTC_ZERO_E}
                              : ctc_zero();
      const CtcME n1 = ctc_lane(full, lane + 1), n2 = ctc_lane(full, lane + 2);
      const CtcME v = ctc_sum3(full, n1, skip_from ? n2 : ctc_zero());
      bt = live ? ctc_norm(v.m, v.e) : ctc_zero();
    }
  }
}

template <typename TG>
__global__ __launch_bounds__(CTC_ROW_THREADS) void ctc_grad_kernel(const float* __restrict__ logits, int64_t ldc,
                                                                   const int64_t* __restrict__ targets, int64_t tstride, int W,
                                                                   int toff, const int* __restrict__ in_len,
                                                                   const int* __restrict__ tgt_len, int blank, CtcWs ws,
                                                                   TG* __restrict__ dl, const float* __restrict__ loss_scale,
                                                                   int B, int T, int C) {
  constexpr int NT = CTC_ROW_THREADS;
  __shared__ float g_s[64], occ_s[CTC_MAX_L + 1], spec[2];
  __shared__ int c_s[64], lcls_s[CTC_MAX_L + 1];
  const int64_t r = blockIdx.x;
  const int b = (int)(r / T), t = (int)(r - (int64_t)b * T), tid = threadIdx.x;
  const float4 info = ws.info[b];
  TG* dr = dl + r * ldc;
  const bool vec = (ldc & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(dl) & (4 * sizeof(TG) - 1)) == 0;
  const int nv = (C + 3) >> 2;
  // (block-uniform; the status is tested first: the lengths of a bad row mean nothing) exact zeros for a bad or
  // infeasible utterance and for the frames past an utterance's end
  if (info.z != 0.f || t >= in_len[b]) {
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
      for (int v = tid; v < nv; v += NT) {
        if (4 * v + 3 < C) ctc_store4<TG>(dr + 4 * v, zero);
        else
          for (int c = 4 * v; c < C; ++c) dr[c] = from_f32<TG>(0.f);
      }
    } else {
      for (int c = tid; c < C; c += NT) dr[c] = from_f32<TG>(0.f);
    }
    return;
  }
  const int L = tgt_len[b], S = 2 * L + 1, SP = 2 * W + 1;
  if (tid < 64) {
    bool badt;
    const int cls = ctc_state_class(targets + (int64_t)b * tstride, tid, S, toff, blank, C, badt);
    float g = 0.f;
    if (tid < S) {
      const float2 a = ws.alpha[r * SP + tid], bb = ws.beta[r * SP + tid];
      g = ctc_posterior(a.x, __float_as_int(a.y), bb.x, __float_as_int(bb.y), info.x, __float_as_int(info.y));
    }
    g_s[tid] = g;
    c_s[tid] = cls;
    const float gb = wave_sum((tid & 1) ? 0.f : g), gl = wave_sum((tid & 1) ? g : 0.f);
    if (tid == 0) { spec[0] = gb; spec[1] = gl; }
  }
  __syncthreads();
  // repeated labels share a class: the first occurrence carries the sum of their posteriors (ascending order), the later
  // ones match no column -- one writer per gradient element
  if (tid < L) {
    const int my = c_s[2 * tid + 1];
    float s = 0.f;
    bool first = true;
    for (int l = 0; l < L; ++l)
      if (c_s[2 * l + 1] == my) {
        s += g_s[2 * l + 1];
        if (l < tid) first = false;
      }
    occ_s[tid] = s;
    lcls_s[tid] = first ? my : -1;
  }
  __syncthreads();
  const float4 rs = ws.rowstat[r];
  const float mx = rs.x, inv = rs.y, offm = rs.z, gb = spec[0], gl = spec[1];
  const float k = (loss_scale ? loss_scale[0] : 1.0f) / ((float)B * (float)max(L, 1));
  auto grad = [&](int c, float z) -> float {
    const float p = ctc_exp(z - mx) * inv;
    float g = p;
    if (c == blank) {
      // softmax[blank] and gamma(blank) both 1 - small under the reference's blank bias: p - gamma from the two small
      // sums, sum_label gamma - sum_{c != blank} softmax_c
      g = p > 0.5f ? gl - offm : p - gb;
    } else {
      for (int j = 0; j < L; ++j)
        if (c == lcls_s[j]) g = p - occ_s[j];
    }
    return g * k;
  };
  const float* zr = logits + r * ldc;
  if (vec) {
    const float4* z4 = reinterpret_cast<const float4*>(zr);
    for (int v = tid; v < nv; v += NT) {
      const float4 q = z4[v];
      const float z[4] = {q.x, q.y, q.z, q.w};
      float g[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) g[i] = 4 * v + i < C ? grad(4 * v + i, z[i]) : 0.f;
      if (4 * v + 3 < C) ctc_store4<TG>(dr + 4 * v, g);
      else
        for (int c = 4 * v; c < C; ++c) dr[c] = from_f32<TG>(g[c - 4 * v]);
    }
  } else {
    for (int c = tid; c < C; c += NT) dr[c] = from_f32<TG>(grad(c, zr[c]));
  }
}

extern "C" int64_t w2v2_ctc_workspace_floats(int B, int T, int target_width) {
  if (B <= 0 || T <= 0 || target_width < 0 || target_width > CTC_MAX_L) return -1;
  return ctc_ws_floats(B, (int64_t)B * T, target_width);
}

extern "C" int w2v2_ctc_fwd_bwd(const float* logits, int64_t ldc, const int64_t* targets, int64_t target_stride,
                                int target_width, int target_offset, const int* input_lengths, const int* target_lengths,
                                int blank, float* loss_rows, void* dlogits, const float* loss_scale, float* workspace,
                                int64_t workspace_floats, int B, int T, int C, int dtype, void* stream) {
  W2V2_REQUIRE(logits && input_lengths && target_lengths && loss_rows && workspace && B > 0 && T > 0 && C > 0 && ldc >= C,
               "ctc: bad arguments");
  W2V2_REQUIRE(target_width >= 0 && target_width <= CTC_MAX_L,
               "ctc: targets of width %d; the lattice of one utterance is one wavefront (at most %d labels)", target_width,
               CTC_MAX_L);
  W2V2_REQUIRE(targets != nullptr || target_width == 0, "ctc: no targets");
  W2V2_REQUIRE(target_stride >= 0 && blank >= 0 && blank < C, "ctc: blank %d outside [0, %d) or a negative target stride",
               blank, C);
  const int64_t rows = (int64_t)B * T;
  W2V2_REQUIRE(rows < (int64_t)1 << 31, "ctc: %lld rows", (long long)rows);
  W2V2_REQUIRE(workspace_floats >= ctc_ws_floats(B, rows, target_width) && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
               "ctc: the workspace needs %lld floats (w2v2_ctc_workspace_floats), 16-byte aligned",
               (long long)ctc_ws_floats(B, rows, target_width));
  const CtcWs ws = ctc_carve(workspace, B, rows, target_width);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ctc_row_kernel, dim3((unsigned)rows), dim3(CTC_ROW_THREADS), 0, st, logits, ldc, targets, target_stride,
                     target_width, target_offset, input_lengths, target_lengths, blank, ws, T, C);
  hipLaunchKernelGGL(ctc_lattice_kernel, dim3(B), dim3(64), 0, st, targets, target_stride, target_width, target_offset,
                     input_lengths, target_lengths, blank, ws, loss_rows, T, C);
  if (dlogits != nullptr) {
    W2V2_DISPATCH_ACT(dtype, "ctc",
      hipLaunchKernelGGL(ctc_grad_kernel<AT>, dim3((unsigned)rows), dim3(CTC_ROW_THREADS), 0, st, logits, ldc, targets,
                         target_stride, target_width, target_offset, input_lengths, target_lengths, blank, ws, (AT*)dlogits,
                         loss_scale, B, T, C););
  }
  W2V2_CHECK_LAUNCH("ctc");
  return 0;
}
