// optim.hip -- fused Adam over one flat f32 parameter arena (torch.optim.Adam semantics,
// ref: config/optim/algo/adam.yaml:1-16, wired at src/main.py:323-335).  One launch updates every
// trainable parameter and refreshes the bf16 copy the MFMA GEMMs read.  HBM-bound:
// 4 f32 streams read (p, g, m, v) + 3 written (p, m, v) + 2 B/param bf16 copy = 30 B/param.
#include "common.h"
#include <stdlib.h>

template <typename TB, int U>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   TB* __restrict__ pb, int64_t n, float lr, float b1, float b2,
                                                   float eps, float step_size, float inv_sqrt_bc2, float gscale,
                                                   const float* __restrict__ scaler, int step, int skip_slot) {
  // dynamic loss scaling (fp16 activations): gradients carry the factor scaler[0]; a step whose gradients held a
  // non-finite value (scaler[1] != 0, set by grad_scaler_check) is skipped as a whole, like torch's GradScaler.step
  if (scaler != nullptr) {
    if (scaler[1] != 0.f) return;
    gscale /= scaler[0];
    // torch's GradScaler skips optimizer.step() on overflow, so Adam's per-parameter step count does NOT advance on a
    // skipped step.  The host counts every call (it never reads the device record); scaler[skip_slot] counts the skipped
    // ones of this parameter range, so the bias corrections are rebuilt here from t = step - skipped.
    if (skip_slot > 0) {
      const float t = fmaxf((float)step - scaler[skip_slot], 1.0f);
      // double pow: at small t, 1 - 0.999^t ~ 1e-3 and the ~1-ulp error of the f32 exp2 / log2 path would be 5e-5..1e-4
      // relative in the correction; once per thread, invisible next to the 30 B/parameter stream.  The
      // host's bias_corr1 / bias_corr2 arguments are NOT used on this path.
      step_size = (float)((double)lr / (1.0 - pow((double)b1, (double)t)));
      inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, (double)t)));
    }
  }
  const int64_t nv = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // U independent 16-byte vectors per thread and pass: 4 U loads in flight per lane before the first use
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < nv; i0 += stride * U) {
    f32x4_hw pp[U], gg[U], mm[U], vv[U];
    // every array is touched once per step: streaming (non-temporal) accesses keep the 30 B/parameter out of the way
    // of the L2 / Infinity Cache contents the next forward wants (the 16-bit operand copy written below)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i < nv) {
        pp[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_hw*>(p) + i);
        gg[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_hw*>(g) + i);
        mm[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_hw*>(m) + i);
        vv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_hw*>(v) + i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i >= nv) break;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gr = gg[u][e] * gscale;
        mm[u][e] = b1 * mm[u][e] + (1.0f - b1) * gr;
        vv[u][e] = b2 * vv[u][e] + (1.0f - b2) * gr * gr;
        const float denom = sqrtf(vv[u][e]) * inv_sqrt_bc2 + eps;
        pp[u][e] -= step_size * mm[u][e] / denom;
      }
      __builtin_nontemporal_store(pp[u], reinterpret_cast<f32x4_hw*>(p) + i);
      __builtin_nontemporal_store(mm[u], reinterpret_cast<f32x4_hw*>(m) + i);
      __builtin_nontemporal_store(vv[u], reinterpret_cast<f32x4_hw*>(v) + i);
      if (pb != nullptr) {
        uint2 w;
        w.x = pack2<TB>(pp[u][0], pp[u][1]);
        w.y = pack2<TB>(pp[u][2], pp[u][3]);
        reinterpret_cast<uint2*>(pb)[i] = w;
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = (nv << 2) + threadIdx.x;
    const float gr = g[i] * gscale;
    const float mi = b1 * m[i] + (1.0f - b1) * gr;
    const float vi = b2 * v[i] + (1.0f - b2) * gr * gr;
    m[i] = mi; v[i] = vi;
    const float pn = p[i] - step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
    p[i] = pn;
    if (pb != nullptr) pb[i] = from_f32<TB>(pn);
  }
}

// ------------------------------------------------------------------------------ dynamic loss scaling (fp16 activations)
// The reference trains under PL `precision: 16` = torch.cuda.amp.GradScaler (config/experiment/
// speaker_wav2vec2_aam.yaml:17): the loss is multiplied by `scale` before backward so that fp16 activation
// gradients stay in range; a step with a non-finite gradient is skipped and the scale halved, and after
// `growth_interval` clean steps it is doubled.  Everything lives in a 4-float device record, so a training step
// never synchronises with the host:  state = {scale, found_inf, growth_tracker, skipped_steps}.
__global__ __launch_bounds__(256) void scaler_check_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ state) {
  const int64_t nv = n >> 2;
  bool bad = false;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    // finite <=> |x| <= FLT_MAX; the sum of absolute values is inf or NaN iff any element is
    const float a = fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
    bad |= !(a <= 3.402823466e38f);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) bad |= !(fabsf(g[(nv << 2) + threadIdx.x]) <= 3.402823466e38f);
  if (__any(bad) && (threadIdx.x & 63) == 0) state[1] = 1.0f;      // benign race: every writer stores the same value
}
__global__ void scaler_update_kernel(float* __restrict__ state, float growth, float backoff, int interval, int ranges) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (state[1] != 0.f) {
    state[0] = fmaxf(state[0] * backoff, 1.0f);
    state[2] = 0.f;
    state[3] += 1.0f;
    if (ranges & 1) state[4] += 1.0f;      // skipped optimiser steps per parameter range (8-float records only)
    if (ranges & 2) state[5] += 1.0f;
  } else {
    state[2] += 1.0f;
    if (state[2] >= (float)interval) {
      state[0] = fminf(state[0] * growth, 16777216.0f);
      state[2] = 0.f;
    }
  }
  state[1] = 0.f;
}

// residual plane of the two-term 16-bit weights: lo = T(p - T(p)) over a table of (offset, count) ranges
template <typename TB>
__global__ __launch_bounds__(256) void weight_residual_kernel(const float* __restrict__ p, TB* __restrict__ lo,
                                                              const int64_t* __restrict__ table) {
  const int64_t off = table[2 * blockIdx.y], n = table[2 * blockIdx.y + 1];
  const int64_t nv = n >> 2;              // ranges are 64-element aligned in the arena; the tail loop covers any rest
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(p + off)[i];
    const float a[4] = {v.x, v.y, v.z, v.w};
    float r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = a[e] - to_f32<TB>(from_f32<TB>(a[e]));
    uint2 w;
    w.x = pack2<TB>(r[0], r[1]);
    w.y = pack2<TB>(r[2], r[3]);
    reinterpret_cast<uint2*>(lo + off)[i] = w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = off + (nv << 2) + threadIdx.x;
    lo[i] = from_f32<TB>(p[i] - to_f32<TB>(from_f32<TB>(p[i])));
  }
}

extern "C" int w2v2_weight_residual(const float* p, void* lo, const int64_t* table, int n_ranges, int dtype,
                                    void* stream) {
  W2V2_REQUIRE(p && lo && table && n_ranges >= 0, "weight_residual: bad arguments");
  if (n_ranges == 0) return 0;
  W2V2_DISPATCH_16(dtype, "weight_residual",
    hipLaunchKernelGGL(weight_residual_kernel<AT>, dim3(64, n_ranges), dim3(256), 0, as_stream(stream), p, (AT*)lo,
                       table););
  W2V2_CHECK_LAUNCH("weight_residual");
  return 0;
}

extern "C" int w2v2_grad_scaler_check(const float* g, int64_t n, float* state, void* stream) {
  W2V2_REQUIRE(g && state && n >= 0, "grad_scaler_check: bad arguments");
  if (n == 0) return 0;
  int64_t nb = cdiv(n >> 2, 256 * 8);
  if (nb > 4096) nb = 4096;
  if (nb < 1) nb = 1;
  hipLaunchKernelGGL(scaler_check_kernel, dim3((unsigned)nb), dim3(256), 0, as_stream(stream), g, n, state);
  W2V2_CHECK_LAUNCH("grad_scaler_check");
  return 0;
}

extern "C" int w2v2_grad_scaler_update(float* state, float growth, float backoff, int growth_interval,
                                       int skipped_ranges, void* stream) {
  W2V2_REQUIRE(state && growth >= 1.f && backoff > 0.f && backoff <= 1.f && growth_interval > 0 &&
                   skipped_ranges >= 0 && skipped_ranges <= 3, "grad_scaler_update: bad arguments");
  hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(64), 0, as_stream(stream), state, growth, backoff,
                     growth_interval, skipped_ranges);
  W2V2_CHECK_LAUNCH("grad_scaler_update");
  return 0;
}

extern "C" int w2v2_adam_step(float* p, const float* g, float* m, float* v, void* pb, int pb_dtype, int64_t n,
                              float lr, float beta1, float beta2, float eps, float bias_corr1, float bias_corr2,
                              float grad_scale, const float* scaler_state, int step, int skip_slot, void* stream) {
  W2V2_REQUIRE(p && g && m && v && n >= 0, "adam_step: bad arguments");
  W2V2_REQUIRE(skip_slot == 0 || ((skip_slot == 4 || skip_slot == 5) && scaler_state != nullptr && step >= 1),
               "adam_step: skip_slot must be 0, or 4 / 5 with an 8-float scaler record and step >= 1");
  W2V2_REQUIRE(bias_corr1 > 0.f && bias_corr2 > 0.f, "adam_step: bias corrections must be > 0");
  if (n == 0) return 0;
  // A/B knobs (tools): W2V2_ADAM_U = vectors per thread and pass (1, 2, 4), W2V2_ADAM_BLOCKS = grid cap
  static const int env_u_raw = getenv("W2V2_ADAM_U") ? atoi(getenv("W2V2_ADAM_U")) : 2;   // 2: 495 vs 549 us over the 99.4 M-parameter arena
  static const int env_u = env_u_raw >= 4 ? 4 : (env_u_raw >= 2 ? 2 : 1);
  // grid cap: none by default (round 6).  The 8192-block cap of round 3 made every thread walk 6 (w2v2-base) to 20
  // (wav2vec2-large) strides of the arena; one pass of one or two vectors per thread measures 456 vs 561 us over the base
  // arena (6.5 vs 5.3 TB/s, tools/adam_sweep.sh, profiles/r06_adam_sweep.txt) and -0.7 % of the step (ABAB x 4).
  static const int env_nb = getenv("W2V2_ADAM_BLOCKS") ? atoi(getenv("W2V2_ADAM_BLOCKS")) : (1 << 20);
  int64_t nb = cdiv(n >> 2, 256 * env_u);
  if (nb > env_nb) nb = env_nb;
  if (nb < 1) nb = 1;
  if (pb == nullptr) pb_dtype = W2V2_BF16;
#define W2V2_ADAM_LAUNCH(U_)                                                                                        \
  hipLaunchKernelGGL((adam_kernel<AT, U_>), dim3((unsigned)nb), dim3(256), 0, as_stream(stream), p, g, m, v, (AT*)pb, n, \
                     lr, beta1, beta2, eps, lr / bias_corr1, 1.0f / sqrtf(bias_corr2), grad_scale, scaler_state, step, skip_slot)
  W2V2_DISPATCH_16(pb_dtype, "adam_step",
    if (env_u == 4) W2V2_ADAM_LAUNCH(4); else if (env_u == 2) W2V2_ADAM_LAUNCH(2); else W2V2_ADAM_LAUNCH(1););
#undef W2V2_ADAM_LAUNCH
  W2V2_CHECK_LAUNCH("adam_step");
  return 0;
}

// ------------------------------------------------------------------------------ gradient accumulation
// PL `trainer.accumulate_grad_batches` = N (ref: config/trainer/trainer.yaml:33): autograd adds the gradient of N
// backward passes into .grad before optimizer.step().  Here every backward WRITES store.grad, so the window's sum lives in
// a second f32 arena: acc = g on the first micro-batch of a window (acc is never read: no zeroing pass, stale NaN / inf
// cannot leak in), acc += g afterwards.  A plain f32 add -- nothing to contract, bit-equal to torch's acc + g; the 1 / N
// of the mean goes into the optimiser's grad_scale.  Same structure as adam_kernel: U independent 16-byte vectors per
// thread and pass, streaming accesses (every byte is touched once per micro-batch), no grid cap, tail on block 0.
// 12 B/parameter (8 on the first micro-batch).
template <int U, bool FIRST>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g,
                                                              int64_t n) {
  const int64_t nv = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < nv; i0 += stride * U) {
    f32x4_hw aa[U], gg[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i < nv) {
        gg[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_hw*>(g) + i);
        if (!FIRST) aa[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_hw*>(acc) + i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i >= nv) break;
      __builtin_nontemporal_store(FIRST ? gg[u] : aa[u] + gg[u], reinterpret_cast<f32x4_hw*>(acc) + i);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = (nv << 2) + threadIdx.x;
    acc[i] = FIRST ? g[i] : acc[i] + g[i];
  }
}

extern "C" int w2v2_grad_accumulate(float* acc, const float* g, int64_t n, int first, void* stream) {
  W2V2_REQUIRE(acc && g && n >= 0, "grad_accumulate: bad arguments");
  W2V2_REQUIRE(((uintptr_t)acc & 15) == 0 && ((uintptr_t)g & 15) == 0,
               "grad_accumulate: acc and g must be 16-byte aligned (arena slices are 64-element aligned)");
  if (n == 0) return 0;
  constexpr int U = 2;                 // adam_kernel's default
  int64_t nb = cdiv(n >> 2, 256 * U);
  if (nb < 1) nb = 1;
  if (first) hipLaunchKernelGGL((grad_accumulate_kernel<U, true>), dim3((unsigned)nb), dim3(256), 0, as_stream(stream), acc, g, n);
  else hipLaunchKernelGGL((grad_accumulate_kernel<U, false>), dim3((unsigned)nb), dim3(256), 0, as_stream(stream), acc, g, n);
  W2V2_CHECK_LAUNCH("grad_accumulate");
  return 0;
}

// ------------------------------------------------------------------------------ global gradient norm (clipping)
// torch.nn.utils.clip_grad_norm_ (PL `trainer.gradient_clip_val`, called after GradScaler.unscale_; ref:
// config/trainer/trainer.yaml) over a slice of the flat f32 gradient arena, in two launches and without atomics: the
// grid is a pure function of n and every reduction runs in a fixed order, so the same bytes give the same bits on
// every launch and on every data-parallel rank (after the all-reduce the replicas hold identical gradients and must
// derive an identical coefficient).  4 B/parameter read; squares accumulate in double.
static constexpr int NORM_THREADS = 256, NORM_U = 4, NORM_MAX_BLOCKS = 1024;
static inline int norm_blocks(int64_t n) {
  int64_t nb = cdiv(n >> 2, (int64_t)NORM_THREADS * NORM_U);
  return (int)(nb < 1 ? 1 : (nb > NORM_MAX_BLOCKS ? NORM_MAX_BLOCKS : nb));
}

__global__ __launch_bounds__(NORM_THREADS) void grad_norm_partial_kernel(const float* __restrict__ g, int64_t n,
                                                                         float gscale, const float* __restrict__ scaler,
                                                                         double* __restrict__ partials) {
  if (scaler != nullptr) gscale /= scaler[0];         // the factor the optimiser kernel applies (unscale + 1/world)
  const int64_t nv = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < nv; i0 += stride * NORM_U) {
    f32x4_hw gg[NORM_U];
#pragma unroll
    for (int u = 0; u < NORM_U; ++u) {
      const int64_t i = i0 + u * stride;
      gg[u] = i < nv ? __builtin_nontemporal_load(reinterpret_cast<const f32x4_hw*>(g) + i) : f32x4_hw{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < NORM_U; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double x = (double)(gg[u][e] * gscale);
        acc = fma(x, x, acc);
      }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const double x = (double)(g[(nv << 2) + threadIdx.x] * gscale);
    acc = fma(x, x, acc);
  }
  // fixed order: shift reduction inside each wavefront, then the four wavefront sums in index order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ double wave_sum[NORM_THREADS / 64];
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = wave_sum[0];
#pragma unroll
    for (int w = 1; w < NORM_THREADS / 64; ++w) s += wave_sum[w];
    partials[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(NORM_THREADS) void grad_norm_final_kernel(const double* __restrict__ partials, int n_partials,
                                                                       float max_norm, float* __restrict__ scaler,
                                                                       float* __restrict__ norm_state) {
  __shared__ double part[NORM_MAX_BLOCKS];
  for (int i = threadIdx.x; i < n_partials; i += blockDim.x) part[i] = partials[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < n_partials; ++i) s += part[i];           // index order
  const float total = (float)sqrt(s);
  const bool finite = fabsf(total) <= 3.402823466e38f;
  float coef = 1.0f;
  if (max_norm > 0.f) coef = fminf(1.0f, max_norm / (total + 1e-6f));
  if (!finite) {
    coef = 0.f;                       // the optimiser kernel skips the step on a zero coefficient
    if (scaler != nullptr) scaler[1] = 1.0f;
  }
  norm_state[0] = total;
  norm_state[1] = coef;
}

extern "C" int w2v2_grad_norm_partials(int64_t n) { return n < 0 ? -1 : norm_blocks(n); }

extern "C" int w2v2_grad_norm(const float* g, int64_t n, float grad_scale, float* scaler_state, float max_norm,
                              double* partials, int n_partials, float* norm_state, void* stream) {
  W2V2_REQUIRE(g && partials && norm_state && n >= 0, "grad_norm: bad arguments");
  const int nb = norm_blocks(n);
  W2V2_REQUIRE(n_partials >= nb, "grad_norm: the partial buffer holds %d doubles, %d needed (w2v2_grad_norm_partials)",
               n_partials, nb);
  hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)nb), dim3(NORM_THREADS), 0, as_stream(stream), g, n,
                     grad_scale, (const float*)scaler_state, partials);
  W2V2_CHECK_LAUNCH("grad_norm (partials)");
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(NORM_THREADS), 0, as_stream(stream), (const double*)partials,
                     nb, max_norm, scaler_state, norm_state);
  W2V2_CHECK_LAUNCH("grad_norm (final)");
  return 0;
}

// ------------------------------------------------------------------------------ general optimiser step
// torch.optim.Adam with L2 weight decay / torch.optim.SGD (ref: config/optim/algo/{adam,sgd}.yaml, built at
// src/main.py:323-335) with the clip coefficient of w2v2_grad_norm folded in: unscale, then clip, then decay, all in
// the one launch.  Same structure as adam_kernel (U vectors per thread, streaming accesses, no grid cap).  SGD keeps its
// momentum buffer in `m` and streams 22 B/parameter (p, g, buf read; p, buf written; 2 B operand copy), 14 without
// momentum.  ALGO: 0 = Adam, 1 = SGD with momentum, 2 = SGD without.  WD = false compiles the decay term out, so that
// instantiation's Adam arithmetic is adam_kernel's.
template <typename TB, int U, int ALGO, bool WD>
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    TB* __restrict__ pb, int64_t n, float lr, float b1, float b2,
                                                    float eps, float step_size, float inv_sqrt_bc2, float gscale, float wd,
                                                    float dampening, int nesterov, const float* __restrict__ norm_state,
                                                    const float* __restrict__ scaler, int step, int skip_slot) {
  float t = (float)step;               // optimiser steps of this range that were not skipped, this one included
  if (scaler != nullptr) {
    if (scaler[1] != 0.f) return;
    gscale /= scaler[0];
    if (skip_slot > 0) {
      t = fmaxf((float)step - scaler[skip_slot], 1.0f);
      if (ALGO == 0) {                 // (see adam_kernel)
        step_size = (float)((double)lr / (1.0 - pow((double)b1, (double)t)));
        inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, (double)t)));
      }
    }
  }
  if (norm_state != nullptr) {
    const float coef = norm_state[1];
    if (coef == 0.f) return;           // non-finite norm: nothing may reach the parameters
    gscale *= coef;
  }
  const bool first = t <= 1.0f;        // torch SGD: momentum_buffer = grad on the first step the parameter takes
  const float keep = 1.0f - dampening;
  const int64_t nv = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < nv; i0 += stride * U) {
    f32x4_hw pp[U], gg[U], mm[U], vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i < nv) {
        pp[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_hw*>(p) + i);
        gg[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_hw*>(g) + i);
        if (ALGO == 0 || (ALGO == 1 && !first)) mm[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_hw*>(m) + i);
        else mm[u] = f32x4_hw{0.f, 0.f, 0.f, 0.f};        // first SGD step: the buffer is written, never read
        if (ALGO == 0) vv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_hw*>(v) + i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i >= nv) break;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float gr = gg[u][e] * gscale;
        if (WD) gr += wd * pp[u][e];
        if (ALGO == 0) {
          mm[u][e] = b1 * mm[u][e] + (1.0f - b1) * gr;
          vv[u][e] = b2 * vv[u][e] + (1.0f - b2) * gr * gr;
          const float denom = sqrtf(vv[u][e]) * inv_sqrt_bc2 + eps;
          pp[u][e] -= step_size * mm[u][e] / denom;
        } else if (ALGO == 1) {
          const float buf = first ? gr : b1 * mm[u][e] + keep * gr;
          mm[u][e] = buf;
          pp[u][e] -= lr * (nesterov ? gr + b1 * buf : buf);
        } else {
          pp[u][e] -= lr * gr;
        }
      }
      __builtin_nontemporal_store(pp[u], reinterpret_cast<f32x4_hw*>(p) + i);
      if (ALGO != 2) __builtin_nontemporal_store(mm[u], reinterpret_cast<f32x4_hw*>(m) + i);
      if (ALGO == 0) __builtin_nontemporal_store(vv[u], reinterpret_cast<f32x4_hw*>(v) + i);
      if (pb != nullptr) {
        uint2 w;
        w.x = pack2<TB>(pp[u][0], pp[u][1]);
        w.y = pack2<TB>(pp[u][2], pp[u][3]);
        reinterpret_cast<uint2*>(pb)[i] = w;
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = (nv << 2) + threadIdx.x;
    float gr = g[i] * gscale;
    if (WD) gr += wd * p[i];
    float pn;
    if (ALGO == 0) {
      const float mi = b1 * m[i] + (1.0f - b1) * gr;
      const float vi = b2 * v[i] + (1.0f - b2) * gr * gr;
      m[i] = mi; v[i] = vi;
      pn = p[i] - step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
    } else if (ALGO == 1) {
      const float buf = first ? gr : b1 * m[i] + keep * gr;
      m[i] = buf;
      pn = p[i] - lr * (nesterov ? gr + b1 * buf : buf);
    } else {
      pn = p[i] - lr * gr;
    }
    p[i] = pn;
    if (pb != nullptr) pb[i] = from_f32<TB>(pn);
  }
}

extern "C" int w2v2_optim_step(int algo, float* p, const float* g, float* m, float* v, void* pb, int pb_dtype, int64_t n,
                               float lr, float beta1, float beta2, float eps, float bias_corr1, float bias_corr2,
                               float grad_scale, float weight_decay, float momentum, float dampening, int nesterov,
                               const float* norm_state, const float* scaler_state, int step, int skip_slot,
                               void* stream) {
  W2V2_REQUIRE(algo == W2V2_OPTIM_ADAM || algo == W2V2_OPTIM_SGD, "optim_step: unknown algorithm %d", algo);
  W2V2_REQUIRE(weight_decay >= 0.f, "optim_step: weight_decay must be >= 0");
  if (algo == W2V2_OPTIM_ADAM && weight_decay == 0.f && norm_state == nullptr)      // the default step: the old entry
    return w2v2_adam_step(p, g, m, v, pb, pb_dtype, n, lr, beta1, beta2, eps, bias_corr1, bias_corr2, grad_scale,
                          scaler_state, step, skip_slot, stream);
  W2V2_REQUIRE(p && g && n >= 0 && step >= 1, "optim_step: bad arguments");
  W2V2_REQUIRE(skip_slot == 0 || ((skip_slot == 4 || skip_slot == 5) && scaler_state != nullptr),
               "optim_step: skip_slot must be 0, or 4 / 5 with an 8-float scaler record");
  const bool wd = weight_decay != 0.f;
  int kind = 0;
  float b1 = beta1;
  if (algo == W2V2_OPTIM_ADAM) {
    W2V2_REQUIRE(m && v && bias_corr1 > 0.f && bias_corr2 > 0.f, "optim_step: Adam needs both moment arenas and bias corrections > 0");
  } else {
    W2V2_REQUIRE(momentum >= 0.f && (!nesterov || (momentum > 0.f && dampening == 0.f)),
                 "optim_step: Nesterov momentum requires a momentum and zero dampening");
    W2V2_REQUIRE(momentum == 0.f || m, "optim_step: SGD with momentum needs the buffer arena");
    kind = momentum != 0.f ? 1 : 2;
    b1 = momentum;
    bias_corr1 = bias_corr2 = 1.f;
  }
  if (n == 0) return 0;
  constexpr int U = 2;                 // adam_kernel's default (profiles/r06_adam_sweep.txt)
  int64_t nb = cdiv(n >> 2, 256 * U);
  if (nb < 1) nb = 1;
  if (pb == nullptr) pb_dtype = W2V2_BF16;
#define W2V2_OPTIM_LAUNCH(ALGO_, WD_)                                                                                  \
  hipLaunchKernelGGL((optim_kernel<AT, U, ALGO_, WD_>), dim3((unsigned)nb), dim3(256), 0, as_stream(stream), p, g, m, v,  \
                     (AT*)pb, n, lr, b1, beta2, eps, lr / bias_corr1, 1.0f / sqrtf(bias_corr2), grad_scale, weight_decay, \
                     dampening, nesterov, norm_state, scaler_state, step, skip_slot)
  W2V2_DISPATCH_16(pb_dtype, "optim_step",
    if (kind == 0) { if (wd) W2V2_OPTIM_LAUNCH(0, true); else W2V2_OPTIM_LAUNCH(0, false); }
    else if (kind == 1) { if (wd) W2V2_OPTIM_LAUNCH(1, true); else W2V2_OPTIM_LAUNCH(1, false); }
    else { if (wd) W2V2_OPTIM_LAUNCH(2, true); else W2V2_OPTIM_LAUNCH(2, false); });
#undef W2V2_OPTIM_LAUNCH
  W2V2_CHECK_LAUNCH("optim_step");
  return 0;
}
