// Learned layer mix (include/w2v2_hip.h, "layer mix"): softmax-weighted sum of the encoder's J hidden states, instance
// normalised over time, written straight into the ECAPA-TDNN feature buffer; its backward (dm, and the gradient of the
// J logits through per-workgroup partials folded in f64); and the scale-add that injects w_j * dm into the encoder's
// running activation gradient.
//
// One geometry for the forward and the backward: grid (B, ceil(H / 64)), 256 threads.  A thread owns the 8 channels
// c0 .. c0 + 7 (c0 = 64 * tile + 8 * (tid & 7)) of the rows t = (tid >> 3) + 32 k: eight lanes cover one 128 B (16-bit) /
// 256 B (f32) row segment with one 16 B / two 16 B loads each.  The forward stages m in LDS ([T][72] f32: 64 channels + 8
// words of padding, so the 8 rows of a wave fall on different banks) -- every element is written and re-read by the
// thread that owns it, so the three statistics passes need no barrier of their own and the hidden states are read once.
// Beyond W2V2_LAYER_MIX_LDS_FRAMES frames the stage is a caller-owned f32 [B * T][H] buffer.  Sums over time: sequential
// per thread, xor-butterfly over the 8 row groups of a wave, then the 4 waves in ascending order: the order depends on
// (n_b, channel) only, which is what makes a row with a length bit-equal to the utterance alone.
#include "common.h"

namespace {

constexpr int MIX_THREADS = 256;
constexpr int MIX_TILE = 64;            // channels per workgroup
constexpr int MIX_ROWS = MIX_THREADS / 8;
constexpr int MIX_LD = MIX_TILE + 8;    // LDS row stride of the staged tile (floats)
constexpr int MIX_MAX_J = W2V2_LAYER_MIX_MAX_STATES;
constexpr int MIX_SMALL = MIX_MAX_J + MIX_THREADS;      // floats of LDS in front of the tile: weights, reduction scratch
constexpr float MIX_EPS = 1e-5f;

// w = softmax(a) (f32, max-subtracted) by the first wave into shw[J]; ends with a barrier
__device__ __forceinline__ void mix_softmax(const float* __restrict__ a, int J, float* shw) {
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    const float v = l < J ? a[l] : -INFINITY;
    const float mx = wave_max(v);
    const float e = l < J ? expf(v - mx) : 0.0f;
    const float s = wave_sum(e);
    if (l < J) shw[l] = e / s;
  }
  __syncthreads();
}

// v[i] (this thread's partial of channel c0 + i) -> the sum over the 32 row groups of the workgroup, in every thread of
// the channel group.  red: 4 * 64 floats of LDS.
__device__ __forceinline__ void mix_colreduce(float (&v)[8], float* red) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] += __shfl_xor(v[i], 8, 64);
    v[i] += __shfl_xor(v[i], 16, 64);
    v[i] += __shfl_xor(v[i], 32, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cg = threadIdx.x & 7;
  __syncthreads();
  if (lane < 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) red[wave * 64 + lane * 8 + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int o = cg * 8 + i;
    v[i] = ((red[o] + red[64 + o]) + red[128 + o]) + red[192 + o];
  }
}

template <typename T> __device__ __forceinline__ void mix_store8(T* p, const float (&v)[8]) {
  Vec8<T> o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o.v[i] = v[i];
  o.store(p);
}

template <typename TX, typename TY, bool NORM, bool LDS_STAGE>
__global__ __launch_bounds__(MIX_THREADS) void layer_mix_fwd_kernel(const void* const* __restrict__ xs,
                                                                    const float* __restrict__ a, int J,
                                                                    const int* __restrict__ lens, TY* __restrict__ y,
                                                                    int64_t ldy, float* __restrict__ rstd,
                                                                    float* __restrict__ w_out, float* __restrict__ stage,
                                                                    int T, int H) {
  extern __shared__ __attribute__((aligned(16))) float mix_smem[];
  float* shw = mix_smem;
  float* red = mix_smem + MIX_MAX_J;
  float* tile = mix_smem + MIX_SMALL;
  const int b = blockIdx.x, cg = threadIdx.x & 7, rg = threadIdx.x >> 3;
  const int c0 = blockIdx.y * MIX_TILE + cg * 8;
  const bool active = c0 < H;
  int n = lens ? lens[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  mix_softmax(a, J, shw);
  if (w_out && b == 0 && blockIdx.y == 0 && (int)threadIdx.x < J) w_out[threadIdx.x] = shw[threadIdx.x];
  const int64_t row0 = (int64_t)b * T;

  auto staged = [&](int t) -> float* {
    if constexpr (LDS_STAGE) return tile + t * MIX_LD + cg * 8;
    else return stage + (row0 + t) * H + c0;
  };
  float sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (active) {
    for (int t = rg; t < n; t += MIX_ROWS) {
      const int64_t off = (row0 + t) * H + c0;
      float m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
      for (int j = 0; j < J; ++j) {
        Vec8<TX> x;
        x.load(static_cast<const TX*>(xs[j]) + off);
        const float w = shw[j];
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = fmaf(w, x.v[i], m[i]);
      }
      if constexpr (NORM) {
        float* s = staged(t);
        *reinterpret_cast<float4*>(s) = make_float4(m[0], m[1], m[2], m[3]);
        *reinterpret_cast<float4*>(s + 4) = make_float4(m[4], m[5], m[6], m[7]);
#pragma unroll
        for (int i = 0; i < 8; ++i) sum[i] += m[i];
      } else {
        mix_store8<TY>(y + (row0 + t) * ldy + c0, m);
      }
    }
  }
  if constexpr (NORM) {
    const float fn = (float)(n > 0 ? n : 1);
    mix_colreduce(sum, red);
    float mu[8], sq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 8; ++i) mu[i] = sum[i] / fn;
    if (active) {
      for (int t = rg; t < n; t += MIX_ROWS) {
        const float* s = staged(t);
        const float4 p = *reinterpret_cast<const float4*>(s), q = *reinterpret_cast<const float4*>(s + 4);
        const float m[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float d = m[i] - mu[i];
          sq[i] = fmaf(d, d, sq[i]);
        }
      }
    }
    mix_colreduce(sq, red);
    float rs[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) rs[i] = 1.0f / sqrtf(sq[i] / fn + MIX_EPS);
    if (active) {
      for (int t = rg; t < n; t += MIX_ROWS) {
        const float* s = staged(t);
        const float4 p = *reinterpret_cast<const float4*>(s), q = *reinterpret_cast<const float4*>(s + 4);
        const float m[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (m[i] - mu[i]) * rs[i];
        mix_store8<TY>(y + (row0 + t) * ldy + c0, o);
      }
      if (rg == 0) mix_store8<float>(rstd + (int64_t)b * H + c0, rs);
    }
  }
  if (active) {          // rows past the utterance's own frames
    const float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = n + rg; t < T; t += MIX_ROWS) mix_store8<TY>(y + (row0 + t) * ldy + c0, z);
  }
}

// the same reduction over the 32 row groups in f64.  red: 4 * 64 doubles of LDS.
__device__ __forceinline__ void mix_colreduce_d(double (&v)[8], double* red) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] += __shfl_xor(v[i], 8, 64);
    v[i] += __shfl_xor(v[i], 16, 64);
    v[i] += __shfl_xor(v[i], 32, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cg = threadIdx.x & 7;
  __syncthreads();
  if (lane < 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) red[wave * 64 + lane * 8 + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int o = cg * 8 + i;
    v[i] = ((red[o] + red[64 + o]) + red[128 + o]) + red[192 + o];
  }
}

// dm = r ((g - s1) - y s2), stored as f32, and this workgroup's partial of d_j = sum dm x_j for every j < J:
// part[wg][MIX_MAX_J] f64.  Where a channel hardly moves over time rstd is as large as 316 and (g - s1) must sum to zero
// over t: a mean rounded to f32, or products summed from the ROUNDED dm, leave an error of 316 ulp-of-g per frame in
// every d_j.  The kernel is bound by its loads (J hidden states per element against one multiply-add each), so the two
// means, dm and the products are carried in f64 -- one f64 fma per element and hidden state -- and only the stored dm
// is rounded.
template <typename TX, typename TG, bool NORM>
__global__ __launch_bounds__(MIX_THREADS) void layer_mix_bwd_kernel(const void* const* __restrict__ xs, int J,
                                                                    const TG* __restrict__ g, int64_t ldg,
                                                                    const TG* __restrict__ y, int64_t ldy,
                                                                    const float* __restrict__ rstd, float* __restrict__ dm,
                                                                    double* __restrict__ part, int T, int H) {
  extern __shared__ __attribute__((aligned(16))) double mix_smem_d[];
  double* red = mix_smem_d;              // 4 * 64 doubles (column sums), then 4 * MIX_MAX_J (the d_j of the four waves)
  const int b = blockIdx.x, cg = threadIdx.x & 7, rg = threadIdx.x >> 3;
  const int c0 = blockIdx.y * MIX_TILE + cg * 8;
  const bool active = c0 < H;
  const int64_t row0 = (int64_t)b * T;
  double s1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float rs[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  if constexpr (NORM) {
    if (active) {
      for (int t = rg; t < T; t += MIX_ROWS) {
        Vec8<TG> gv, yv;
        gv.load(g + (row0 + t) * ldg + c0);
        yv.load(y + (row0 + t) * ldy + c0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          s1[i] += (double)gv.v[i];
          s2[i] = fma((double)gv.v[i], (double)yv.v[i], s2[i]);
        }
      }
      Vec8<float> r;
      r.load(rstd + (int64_t)b * H + c0);
#pragma unroll
      for (int i = 0; i < 8; ++i) rs[i] = r.v[i];
    }
    mix_colreduce_d(s1, red);
    mix_colreduce_d(s2, red);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s1[i] /= (double)T;
      s2[i] /= (double)T;
    }
  }
  double acc[MIX_MAX_J];
#pragma unroll
  for (int j = 0; j < MIX_MAX_J; ++j) acc[j] = 0.0;
  if (active) {
    for (int t = rg; t < T; t += MIX_ROWS) {
      Vec8<TG> gv;
      gv.load(g + (row0 + t) * ldg + c0);
      double d[8];
      if constexpr (NORM) {
        Vec8<TG> yv;
        yv.load(y + (row0 + t) * ldy + c0);
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = (double)rs[i] * (((double)gv.v[i] - s1[i]) - (double)yv.v[i] * s2[i]);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = (double)gv.v[i];
      }
      const int64_t off = (row0 + t) * H + c0;
      float df[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) df[i] = (float)d[i];
      mix_store8<float>(dm + off, df);
#pragma unroll
      for (int j = 0; j < MIX_MAX_J; ++j) {
        if (j < J) {
          Vec8<TX> x;
          x.load(static_cast<const TX*>(xs[j]) + off);
          double p = acc[j];
#pragma unroll
          for (int i = 0; i < 8; ++i) p = fma(d[i], (double)x.v[i], p);
          acc[j] = p;
        }
      }
    }
  }
  // the threads' partials: butterfly over the wave, the four waves in ascending order (the logits' gradient is a
  // difference of nearly equal d_j: hidden states of neighbouring layers are alike)
  double* dred = red + 4 * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < MIX_MAX_J; ++j) {
    if (j < J) {
      const double s = wave_sum_d(acc[j]);
      if (lane == 0) dred[wave * MIX_MAX_J + j] = s;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < MIX_MAX_J) {
    const int j = threadIdx.x;
    const double s = j < J ? ((dred[j] + dred[MIX_MAX_J + j]) + dred[2 * MIX_MAX_J + j]) + dred[3 * MIX_MAX_J + j] : 0.0;
    part[((int64_t)b * gridDim.y + blockIdx.y) * MIX_MAX_J + j] = s;
  }
}

// d_j = sum over the workgroup partials in ascending order per lane, butterfly over the lanes, all in f64;
// grad[j] += w_j (d_j - sum_k w_k d_k).  One workgroup of 1024 threads.
__global__ __launch_bounds__(1024) void layer_mix_fold_kernel(const double* __restrict__ part, int nwg,
                                                              const float* __restrict__ a, int J,
                                                              float* __restrict__ grad) {
  __shared__ double d[MIX_MAX_J];
  __shared__ float shw[MIX_MAX_J];
  mix_softmax(a, J, shw);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < J; j += 16) {
    double s = 0.0;
    for (int i = lane; i < nwg; i += 64) s += part[(int64_t)i * MIX_MAX_J + j];
    s = wave_sum_d(s);
    if (lane == 0) d[j] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < J) {
    double all = 0.0;
    for (int k = 0; k < J; ++k) all += (double)shw[k] * d[k];
    const int j = threadIdx.x;
    grad[j] += (float)((double)shw[j] * (d[j] - all));
  }
}

// G = (overwrite ? 0 : G) + (sum_{j = lo .. hi} w_j) dm, 8 elements per lane
template <typename TG, typename TD>
__global__ __launch_bounds__(256) void scale_add_kernel(TG* __restrict__ G, const TD* __restrict__ dm,
                                                        const float* __restrict__ w, int lo, int hi, int overwrite,
                                                        int64_t n8) {
  float s = 0.0f;
  for (int j = lo; j <= hi; ++j) s += w[j];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    Vec8<TD> d;
    d.load(dm + i * 8);
    Vec8<TG> o;
    if (overwrite) {
#pragma unroll
      for (int k = 0; k < 8; ++k) o.v[k] = s * d.v[k];
    } else {
      o.load(G + i * 8);
#pragma unroll
      for (int k = 0; k < 8; ++k) o.v[k] = fmaf(s, d.v[k], o.v[k]);
    }
    o.store(G + i * 8);
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int mix_check_shape(const char* name, int B, int T, int H, int J) {
  W2V2_REQUIRE(B >= 1 && T >= 1 && H >= 8 && H % 8 == 0, "%s: B >= 1, T >= 1 and H a positive multiple of 8 (got B %d, T %d, H %d)",
               name, B, T, H);
  W2V2_REQUIRE(J >= 1 && J <= MIX_MAX_J, "%s: 1 <= J <= %d hidden states (got %d)", name, MIX_MAX_J, J);
  W2V2_REQUIRE((int64_t)B * T * H < ((int64_t)1 << 40) && cdiv(H, MIX_TILE) <= 65535, "%s: shape out of range", name);
  return 0;
}

template <typename TX, typename TY>
int launch_fwd(const void* const* xs, const float* a, int J, const int* lens, void* y, int64_t ldy, float* rstd, float* w_out,
               float* stage, int B, int T, int H, bool norm, hipStream_t st) {
  const dim3 grid(B, (unsigned)cdiv(H, MIX_TILE)), block(MIX_THREADS);
  const bool lds_stage = norm && T <= W2V2_LAYER_MIX_LDS_FRAMES;
  const size_t small = MIX_SMALL * sizeof(float);
  if (!norm)
    return w2v2_launch_lds<layer_mix_fwd_kernel<TX, TY, false, false>>("w2v2_layer_mix_fwd", grid, block, small, st, xs, a, J,
                                                                      lens, (TY*)y, ldy, rstd, w_out, stage, T, H);
  if (lds_stage)
    return w2v2_launch_lds<layer_mix_fwd_kernel<TX, TY, true, true>>("w2v2_layer_mix_fwd", grid, block,
                                                                    small + (size_t)T * MIX_LD * sizeof(float), st, xs, a, J,
                                                                    lens, (TY*)y, ldy, rstd, w_out, stage, T, H);
  return w2v2_launch_lds<layer_mix_fwd_kernel<TX, TY, true, false>>("w2v2_layer_mix_fwd", grid, block, small, st, xs, a, J,
                                                                   lens, (TY*)y, ldy, rstd, w_out, stage, T, H);
}

}  // namespace

extern "C" {

int w2v2_layer_mix_fwd(const void* const* xs, const float* logits, int J, const int* lens, void* y, int64_t ldy, float* rstd,
                       float* w_out, float* stage, int B, int T, int H, int instance_norm, int dtype_x, int dtype_y,
                       void* stream) {
  const char* name = "w2v2_layer_mix_fwd";
  if (mix_check_shape(name, B, T, H, J)) return -1;
  W2V2_REQUIRE(xs && logits && y, "%s: null pointer", name);
  W2V2_REQUIRE(dtype_y == W2V2_F32 || dtype_y == W2V2_BF16, "%s: y is f32 or bf16 (got dtype %d)", name, dtype_y);
  W2V2_REQUIRE(ldy >= H && ldy % 8 == 0 && aligned16(y), "%s: y needs a row stride >= H that is a multiple of 8 and a 16-byte aligned base", name);
  if (instance_norm) {
    W2V2_REQUIRE(rstd && aligned16(rstd), "%s: instance_norm needs a 16-byte aligned rstd [B][H]", name);
    W2V2_REQUIRE(T <= W2V2_LAYER_MIX_LDS_FRAMES || (stage && aligned16(stage)),
                 "%s: more than %d frames need a 16-byte aligned f32 stage [B * T][H]", name, W2V2_LAYER_MIX_LDS_FRAMES);
  }
  const hipStream_t st = as_stream(stream);
  int rc = 0;
  W2V2_DISPATCH_ACT(dtype_x, name, {
    if (dtype_y == W2V2_F32)
      rc = launch_fwd<AT, float>(xs, logits, J, lens, y, ldy, rstd, w_out, stage, B, T, H, instance_norm != 0, st);
    else
      rc = launch_fwd<AT, bf16_t>(xs, logits, J, lens, y, ldy, rstd, w_out, stage, B, T, H, instance_norm != 0, st);
  });
  if (rc) return rc;
  W2V2_CHECK_LAUNCH(name);
  return 0;
}

int64_t w2v2_layer_mix_workspace_floats(int B, int T, int H, int J) {
  if (B < 1 || T < 1 || H < 8 || H % 8 || J < 1 || J > MIX_MAX_J) return -1;
  return (int64_t)B * cdiv(H, MIX_TILE) * MIX_MAX_J * 2;      // one f64 per workgroup and logit
}

int w2v2_layer_mix_bwd(const void* const* xs, const float* logits, int J, const void* g, int64_t ldg, const void* y,
                       int64_t ldy, const float* rstd, float* dm, float* grad_logits, float* workspace, int B, int T, int H,
                       int instance_norm, int dtype_x, int dtype_g, void* stream) {
  const char* name = "w2v2_layer_mix_bwd";
  if (mix_check_shape(name, B, T, H, J)) return -1;
  W2V2_REQUIRE(xs && logits && g && dm && grad_logits && workspace, "%s: null pointer", name);
  W2V2_REQUIRE(dtype_g == W2V2_F32 || dtype_g == W2V2_BF16, "%s: g and y are f32 or bf16 (got dtype %d)", name, dtype_g);
  W2V2_REQUIRE(ldg >= H && ldg % 8 == 0 && aligned16(g) && aligned16(dm) && aligned16(workspace),
               "%s: g needs a row stride >= H that is a multiple of 8; g, dm and workspace 16-byte aligned bases", name);
  if (instance_norm)
    W2V2_REQUIRE(y && rstd && ldy >= H && ldy % 8 == 0 && aligned16(y) && aligned16(rstd),
                 "%s: instance_norm needs y (row stride >= H, a multiple of 8) and rstd, 16-byte aligned", name);
  const hipStream_t st = as_stream(stream);
  double* ws = reinterpret_cast<double*>(workspace);
  const dim3 grid(B, (unsigned)cdiv(H, MIX_TILE)), block(MIX_THREADS);
  const size_t lds = (4 * 64 + 4 * MIX_MAX_J) * sizeof(double);
  W2V2_DISPATCH_ACT(dtype_x, name, {
    if (dtype_g == W2V2_F32) {
      if (instance_norm)
        hipLaunchKernelGGL((layer_mix_bwd_kernel<AT, float, true>), grid, block, lds, st, xs, J, (const float*)g, ldg,
                           (const float*)y, ldy, rstd, dm, ws, T, H);
      else
        hipLaunchKernelGGL((layer_mix_bwd_kernel<AT, float, false>), grid, block, lds, st, xs, J, (const float*)g, ldg,
                           (const float*)y, ldy, rstd, dm, ws, T, H);
    } else {
      if (instance_norm)
        hipLaunchKernelGGL((layer_mix_bwd_kernel<AT, bf16_t, true>), grid, block, lds, st, xs, J, (const bf16_t*)g, ldg,
                           (const bf16_t*)y, ldy, rstd, dm, ws, T, H);
      else
        hipLaunchKernelGGL((layer_mix_bwd_kernel<AT, bf16_t, false>), grid, block, lds, st, xs, J, (const bf16_t*)g, ldg,
                           (const bf16_t*)y, ldy, rstd, dm, ws, T, H);
    }
  });
  W2V2_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(layer_mix_fold_kernel, dim3(1), dim3(1024), 0, st, ws, (int)(B * cdiv(H, MIX_TILE)), logits, J,
                     grad_logits);
  W2V2_CHECK_LAUNCH(name);
  return 0;
}

int w2v2_scale_add(void* G, const void* dm, const float* w, int lo, int hi, int overwrite, int64_t n, int dtype_g,
                   int dtype_dm, void* stream) {
  const char* name = "w2v2_scale_add";
  W2V2_REQUIRE(G && dm && w, "%s: null pointer", name);
  W2V2_REQUIRE(n >= 8 && n % 8 == 0, "%s: n must be a positive multiple of 8 (got %lld)", name, (long long)n);
  W2V2_REQUIRE(lo >= 0 && hi >= lo && hi < MIX_MAX_J, "%s: 0 <= lo <= hi < %d (got %d .. %d)", name, MIX_MAX_J, lo, hi);
  W2V2_REQUIRE(dtype_dm == W2V2_F32 || dtype_dm == W2V2_BF16, "%s: dm is f32 or bf16 (got dtype %d)", name, dtype_dm);
  W2V2_REQUIRE(aligned16(G) && aligned16(dm), "%s: G and dm need 16-byte aligned bases", name);
  const int64_t n8 = n / 8;
  const int blocks = (int)(cdiv(n8, 256) < 4096 ? cdiv(n8, 256) : 4096);
  const hipStream_t st = as_stream(stream);
  W2V2_DISPATCH_ACT(dtype_g, name, {
    if (dtype_dm == W2V2_F32)
      hipLaunchKernelGGL((scale_add_kernel<AT, float>), dim3(blocks), dim3(256), 0, st, (AT*)G, (const float*)dm, w, lo, hi,
                         overwrite, n8);
    else
      hipLaunchKernelGGL((scale_add_kernel<AT, bf16_t>), dim3(blocks), dim3(256), 0, st, (AT*)G, (const bf16_t*)dm, w, lo, hi,
                         overwrite, n8);
  });
  W2V2_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
