// Waveform augmentation on the device (f32, gfx950, wave64): the `augmenter` stage between the chunk selector and
// fbank.hip.  include/w2v2_hip.h, "waveform augmentation", is the definition of every operation here; the random draws
// are the host's (data/augment.py), the kernels take their results as small device tables.
//   w2v2_aug_time_dropout   zero S spans per listed row (in place)
//   w2v2_aug_mix_uniform    y = c x + (1 - c) u, u from the counter hash of common.h (in place)
//   w2v2_aug_mix_bank       the same with u = a noise bank row repeated to the utterance's length (in place)
//   w2v2_aug_fir            per-row zero-phase FIR of up to W2V2_AUG_MAX_TAPS taps (src -> dst): the hot kernel
//   w2v2_aug_resample       rational resampling U / D through a prototype low-pass (src -> dst)
// Variable lengths: a sample at index >= len is zero by INDEX, every output is one chain of fmas whose order depends on
// the output's position in its own row and on that row's parameters alone -- tiles start at multiples of the tile size of
// the row, nothing depends on B, N, R or the grid -- so a row is bit-identical to the same call on the row alone.
// No atomics, one writer per element, row * ld in 64 bits, nothing allocated, everything on the caller's stream.
#include "common.h"

namespace {

__device__ __forceinline__ float aug_qnan() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ int aug_len(const int* __restrict__ lens, int row, int N) {
  return lens ? min(max(lens[row], 0), N) : N;
}

// ------------------------------------------------------------------------------------------ elementwise, in place
// A thread owns 4 consecutive samples of one listed row and decides per sample whether to rewrite it; a sample that
// keeps its value is neither read nor written by the dropout.  The 16-byte forms are taken when all four samples are
// rewritten and the address allows it; what is stored is the same either way.
constexpr int EW_THREADS = 256, EW_PER = 4, EW_TILE = EW_THREADS * EW_PER;

__device__ __forceinline__ bool aug_vec_ok(const float* p, int i0, int N) { return i0 + EW_PER <= N && ((uintptr_t)p & 15) == 0; }

__global__ __launch_bounds__(EW_THREADS) void aug_time_dropout_kernel(float* __restrict__ x, int64_t ld, int N,
                                                                      const int* __restrict__ lens, const int* __restrict__ rows,
                                                                      const int* __restrict__ spans, int S) {
  const int r = blockIdx.y, row = rows[r];
  const int i0 = (blockIdx.x * EW_THREADS + threadIdx.x) * EW_PER;
  if (i0 >= N) return;
  const int len = aug_len(lens, row, N);
  unsigned zero = 0;                                        // bit k: sample i0 + k becomes 0
#pragma unroll
  for (int k = 0; k < EW_PER; ++k) zero |= (i0 + k >= len) ? 1u << k : 0u;
  const int* sp = spans + (int64_t)r * S * 2;
  for (int s = 0; s < S; ++s) {
    const int64_t a = sp[2 * s], b = a + (int64_t)sp[2 * s + 1];     // [a, b): empty when the length is <= 0
#pragma unroll
    for (int k = 0; k < EW_PER; ++k) zero |= (i0 + k >= a && i0 + k < b) ? 1u << k : 0u;
  }
  float* p = x + (int64_t)row * ld + i0;
  if (zero == 15u && aug_vec_ok(p, i0, N)) {
    *reinterpret_cast<float4*>(p) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
#pragma unroll
  for (int k = 0; k < EW_PER; ++k)
    if ((zero >> k & 1u) && i0 + k < N) p[k] = 0.0f;
}

// u in [0, 1): the top 24 bits of one hash per sample
__device__ __forceinline__ float aug_uniform(uint32_t key, int i) { return (float)(rng_pair(key, (uint64_t)i) >> 8) * 0x1p-24f; }

template <bool BANK>
__global__ __launch_bounds__(EW_THREADS) void aug_mix_kernel(float* __restrict__ x, int64_t ld, int N, const int* __restrict__ lens,
                                                             const int* __restrict__ rows, const float* __restrict__ coef,
                                                             uint64_t seed, const float* __restrict__ bank, int64_t ld_bank,
                                                             const int* __restrict__ bank_lens, int M,
                                                             const int* __restrict__ bank_row) {
  const int r = blockIdx.y, row = rows[r];
  const int i0 = (blockIdx.x * EW_THREADS + threadIdx.x) * EW_PER;
  if (i0 >= N) return;
  const int len = aug_len(lens, row, N);
  const float c = coef[r], omc = 1.0f - c;
  uint32_t key = 0;
  const float* nz = nullptr;
  int L = 0;
  bool bad = false;
  if constexpr (BANK) {
    const int m = bank_row[r];
    bad = m < 0 || m >= M;
    if (!bad) {
      L = bank_lens[m];
      bad = L < 1 || L > ld_bank;
      nz = bank + (int64_t)m * ld_bank;
    }
  } else {
    key = rng_key(((uint64_t)(uint32_t)row << 32) | rng_key(seed));
  }
  float* p = x + (int64_t)row * ld + i0;
  const bool vec = aug_vec_ok(p, i0, N);
  float v[EW_PER];
  if (vec) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else {
#pragma unroll
    for (int k = 0; k < EW_PER; ++k) v[k] = i0 + k < N ? p[k] : 0.0f;
  }
  int ph = BANK && !bad ? i0 % L : 0;                       // i mod L without a division per sample
#pragma unroll
  for (int k = 0; k < EW_PER; ++k) {
    const int i = i0 + k;
    float u;
    if constexpr (BANK) {
      u = (bad || i >= len) ? 0.0f : nz[ph];
      if (++ph >= L) ph = 0;
    } else {
      u = aug_uniform(key, i);
    }
    v[k] = i >= len ? 0.0f : (bad ? aug_qnan() : fmaf(c, v[k], omc * u));
  }
  if (vec) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < EW_PER; ++k)
      if (i0 + k < N) p[k] = v[k];
  }
}

// ------------------------------------------------------------------------------------------ FIR
// One workgroup per (tile of FIR_TILE outputs, listed row).  With P = (K - 1) / 2 and the taps staged reversed,
// hr[i] = h[K - 1 - i], output o of the tile is  sum_i hr[i] xs[o + i]  over the staged samples xs[p] = x[tile0 - P + p]:
// ascending i = descending j, for every output alike.  A thread owns outputs o0 .. o0 + 7 (o0 = 8 tid) and keeps
// xs[o0 + i .. o0 + i + 12) in registers; a step of four taps reads one float4 of samples and one float4 of taps (the
// same address in every lane: a broadcast) for 32 fmas, then the window moves on by four.  K is rounded up to a multiple
// of four with zero taps, and the samples only those taps meet are staged as zeros, so the padding adds exact zeros.
// LDS image of the samples: 4 floats of padding behind every 64 (the threads of a wave read 16-byte pieces 32 bytes
// apart: unpadded, lanes l and l + 8 would meet on one bank); an aligned float4 never straddles a pad.
constexpr int FIR_THREADS = 256, FIR_PER = 8, FIR_TILE = FIR_THREADS * FIR_PER;
constexpr int FIR_K4 = (W2V2_AUG_MAX_TAPS + 3) / 4 * 4;
constexpr int FIR_XS = FIR_TILE + FIR_K4;                  // staged samples at the largest tap count
__host__ __device__ constexpr int fir_xi(int p) { return p + ((p >> 6) << 2); }
static_assert(W2V2_AUG_MAX_TAPS % 2 == 1 && W2V2_AUG_MAX_TAPS >= 2561, "an odd cap of at least 2,561 taps");
static_assert((fir_xi(FIR_XS) + 4 + FIR_K4) * 4 <= 64 * 1024, "samples and taps fit the static LDS of a workgroup");

__global__ __launch_bounds__(FIR_THREADS) void aug_fir_kernel(const float* __restrict__ src, int64_t ld_src, int N_in,
                                                              const int* __restrict__ lens, const int* __restrict__ src_rows,
                                                              float* __restrict__ dst, int64_t ld_dst, int N_out,
                                                              const int* __restrict__ dst_rows, const float* __restrict__ taps,
                                                              int64_t ldt, const int* __restrict__ ntaps) {
  __shared__ __attribute__((aligned(16))) float xs[fir_xi(FIR_XS) + 4];
  __shared__ __attribute__((aligned(16))) float hr[FIR_K4];
  const int tid = threadIdx.x, r = blockIdx.y, tile0 = blockIdx.x * FIR_TILE;
  const int srow = src_rows[r], drow = dst_rows[r];
  const int len = aug_len(lens, srow, N_in);
  const int K = ntaps[r];
  const bool bad = K < 1 || K > W2V2_AUG_MAX_TAPS || (K & 1) == 0 || K > ldt;
  float* __restrict__ y = dst + (int64_t)drow * ld_dst;
  const int o0 = tid * FIR_PER, n0 = tile0 + o0;
  const int live = min(len, N_out);                         // outputs [0, live) are sums, [live, N_out) zeros
  if (bad || tile0 >= live) {                               // (workgroup-uniform)
    const float fill = bad ? aug_qnan() : 0.0f;
#pragma unroll
    for (int k = 0; k < FIR_PER; ++k)
      if (n0 + k < N_out) y[n0 + k] = fill;
    return;
  }
  const int P = (K - 1) >> 1, K4 = (K + 3) & ~3, need = FIR_TILE + K4;
  const float* __restrict__ h = taps + (int64_t)r * ldt;
  for (int i = tid; i < K4; i += FIR_THREADS) hr[i] = i < K ? h[K - 1 - i] : 0.0f;
  const float* __restrict__ x = src + (int64_t)srow * ld_src;
  for (int p = tid; p < need; p += FIR_THREADS) {
    const int64_t s = (int64_t)tile0 - P + p;
    xs[fir_xi(p)] = (p < FIR_TILE + K - 1 && s >= 0 && s < len) ? x[s] : 0.0f;
  }
  __syncthreads();

  float acc[FIR_PER], w[FIR_PER + 4];
#pragma unroll
  for (int k = 0; k < FIR_PER; ++k) acc[k] = 0.0f;
  {
    const float4 a = *reinterpret_cast<const float4*>(xs + fir_xi(o0)), b = *reinterpret_cast<const float4*>(xs + fir_xi(o0 + 4));
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
  }
#pragma unroll 4
  for (int i = 0; i < K4; i += 4) {
    const float4 hv = *reinterpret_cast<const float4*>(hr + i);
    const float4 nx = *reinterpret_cast<const float4*>(xs + fir_xi(o0 + i + FIR_PER));
    w[8] = nx.x; w[9] = nx.y; w[10] = nx.z; w[11] = nx.w;
    const float h4[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int k = 0; k < FIR_PER; ++k) acc[k] = fmaf(h4[t], w[k + t], acc[k]);
#pragma unroll
    for (int k = 0; k < FIR_PER; ++k) w[k] = w[k + 4];
  }
#pragma unroll
  for (int k = 0; k < FIR_PER; ++k)
    if (n0 + k >= live) acc[k] = 0.0f;
  if (n0 + FIR_PER <= N_out && ((uintptr_t)(y + n0) & 15) == 0) {
    *reinterpret_cast<float4*>(y + n0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4*>(y + n0 + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
  } else {
#pragma unroll
    for (int k = 0; k < FIR_PER; ++k)
      if (n0 + k < N_out) y[n0 + k] = acc[k];
  }
}

// ------------------------------------------------------------------------------------------ resample
// One output per thread: about 2 half / U + 1 taps (65 at 20/19), each a sample of the row and a tap of the prototype
// out of the cache.  Tap index of sample j for output m: t = m D + half - j U, walked with ascending j.
constexpr int RS_THREADS = 256;

__global__ __launch_bounds__(RS_THREADS) void aug_resample_kernel(const float* __restrict__ src, int64_t ld_src, int N_in,
                                                                  const int* __restrict__ lens, const int* __restrict__ src_rows,
                                                                  float* __restrict__ dst, int64_t ld_dst, int N_out,
                                                                  const int* __restrict__ dst_rows, int* __restrict__ out_lens,
                                                                  int U, int D, const float* __restrict__ h, int half) {
  const int r = blockIdx.y, srow = src_rows[r], drow = dst_rows[r];
  const int m = blockIdx.x * RS_THREADS + threadIdx.x;
  const int len = aug_len(lens, srow, N_in);
  const int64_t full = ((int64_t)len * U + D - 1) / D;
  const int out_len = (int)(full < N_out ? full : N_out);
  if (m == 0 && out_lens) out_lens[drow] = out_len;
  if (m >= N_out) return;
  const float* __restrict__ x = src + (int64_t)srow * ld_src;
  float v = 0.0f;
  if (m < out_len) {
    if (U == D) {
      v = x[m];
    } else {
      const int64_t c = (int64_t)m * D + half;               // tap index of sample 0
      const int64_t lo = c - 2 * (int64_t)half;              // j U >= lo
      const int64_t j_lo = lo > 0 ? (lo + U - 1) / U : 0, j_hi = min(c / U, (int64_t)len - 1);
      float acc = 0.0f;
      for (int64_t j = j_lo; j <= j_hi; ++j) acc = fmaf(x[j], h[c - j * U], acc);
      v = (float)U * acc;
    }
  }
  dst[(int64_t)drow * ld_dst + m] = v;
}

bool aug_buf_ok(const void* p, int64_t ld, int N) { return p && N >= 1 && N <= (1 << 30) && ld >= N; }
constexpr int AUG_MAX_ROWS = 65535;                         // gridDim.y

}  // namespace

extern "C" int w2v2_aug_time_dropout(float* x, int64_t ld, int N, const int32_t* lens, const int32_t* rows, int R,
                                     const int32_t* spans, int S, void* stream) {
  W2V2_REQUIRE(aug_buf_ok(x, ld, N) && rows && R >= 1 && R <= AUG_MAX_ROWS && S >= 0 && (S == 0 || spans),
               "aug_time_dropout: bad arguments (x [rows][ld >= N >= 1], a row list of 1..65535 entries, spans [R][S][2])");
  hipLaunchKernelGGL(aug_time_dropout_kernel, dim3((unsigned)cdiv(N, EW_TILE), (unsigned)R), dim3(EW_THREADS), 0, as_stream(stream),
                     x, ld, N, lens, rows, spans, S);
  W2V2_CHECK_LAUNCH("aug_time_dropout");
  return 0;
}

extern "C" int w2v2_aug_mix_uniform(float* x, int64_t ld, int N, const int32_t* lens, const int32_t* rows, int R,
                                    const float* coef, int64_t seed, void* stream) {
  W2V2_REQUIRE(aug_buf_ok(x, ld, N) && rows && coef && R >= 1 && R <= AUG_MAX_ROWS,
               "aug_mix_uniform: bad arguments (x [rows][ld >= N >= 1], a row list of 1..65535 entries, coef [R])");
  hipLaunchKernelGGL(aug_mix_kernel<false>, dim3((unsigned)cdiv(N, EW_TILE), (unsigned)R), dim3(EW_THREADS), 0, as_stream(stream), x,
                     ld, N, lens, rows, coef, (uint64_t)seed, (const float*)nullptr, (int64_t)0, (const int*)nullptr, 0, (const int*)nullptr);
  W2V2_CHECK_LAUNCH("aug_mix_uniform");
  return 0;
}

extern "C" int w2v2_aug_mix_bank(float* x, int64_t ld, int N, const int32_t* lens, const int32_t* rows, int R, const float* coef,
                                 const float* bank, int64_t ld_bank, const int32_t* bank_lens, int M, const int32_t* bank_row,
                                 void* stream) {
  W2V2_REQUIRE(aug_buf_ok(x, ld, N) && rows && coef && R >= 1 && R <= AUG_MAX_ROWS,
               "aug_mix_bank: bad arguments (x [rows][ld >= N >= 1], a row list of 1..65535 entries, coef [R])");
  W2V2_REQUIRE(bank && bank_lens && bank_row && M >= 1 && ld_bank >= 1,
               "aug_mix_bank: bank [M >= 1][ld_bank >= 1], bank_lens [M] and bank_row [R] must be set");
  hipLaunchKernelGGL(aug_mix_kernel<true>, dim3((unsigned)cdiv(N, EW_TILE), (unsigned)R), dim3(EW_THREADS), 0, as_stream(stream), x,
                     ld, N, lens, rows, coef, (uint64_t)0, bank, ld_bank, bank_lens, M, bank_row);
  W2V2_CHECK_LAUNCH("aug_mix_bank");
  return 0;
}

extern "C" int w2v2_aug_fir_tile(void) { return FIR_TILE; }

extern "C" int w2v2_aug_fir(const float* src, int64_t ld_src, int N_in, const int32_t* lens, const int32_t* src_rows, float* dst,
                            int64_t ld_dst, int N_out, const int32_t* dst_rows, int R, const float* taps, int64_t ldt,
                            const int32_t* ntaps, void* stream) {
  W2V2_REQUIRE(aug_buf_ok(src, ld_src, N_in) && aug_buf_ok(dst, ld_dst, N_out) && src_rows && dst_rows && R >= 1 && R <= AUG_MAX_ROWS,
               "aug_fir: bad arguments (src [rows][ld_src >= N_in >= 1], dst [rows][ld_dst >= N_out >= 1], two row lists of "
               "1..65535 entries)");
  W2V2_REQUIRE(src != dst, "aug_fir: src and dst must not be the same buffer");
  W2V2_REQUIRE(taps && ntaps && ldt >= 1, "aug_fir: taps [R][ldt >= 1] and ntaps [R] must be set");
  hipLaunchKernelGGL(aug_fir_kernel, dim3((unsigned)cdiv(N_out, FIR_TILE), (unsigned)R), dim3(FIR_THREADS), 0, as_stream(stream), src,
                     ld_src, N_in, lens, src_rows, dst, ld_dst, N_out, dst_rows, taps, ldt, ntaps);
  W2V2_CHECK_LAUNCH("aug_fir");
  return 0;
}

extern "C" int w2v2_aug_resample_tile(void) { return RS_THREADS; }

extern "C" int w2v2_aug_resample(const float* src, int64_t ld_src, int N_in, const int32_t* lens, const int32_t* src_rows,
                                 float* dst, int64_t ld_dst, int N_out, const int32_t* dst_rows, int32_t* out_lens, int R, int U,
                                 int D, const float* h, int half, void* stream) {
  W2V2_REQUIRE(aug_buf_ok(src, ld_src, N_in) && aug_buf_ok(dst, ld_dst, N_out) && src_rows && dst_rows && R >= 1 && R <= AUG_MAX_ROWS,
               "aug_resample: bad arguments (src [rows][ld_src >= N_in >= 1], dst [rows][ld_dst >= N_out >= 1], two row lists "
               "of 1..65535 entries)");
  W2V2_REQUIRE(src != dst, "aug_resample: src and dst must not be the same buffer");
  W2V2_REQUIRE(U >= 1 && U <= 4096 && D >= 1 && D <= 4096, "aug_resample: U = %d, D = %d outside [1, 4096]", U, D);
  W2V2_REQUIRE(U == D || (h && half >= 0 && half <= (1 << 20)), "aug_resample: h [2 half + 1] with 0 <= half <= 2^20 must be set");
  hipLaunchKernelGGL(aug_resample_kernel, dim3((unsigned)cdiv(N_out, RS_THREADS), (unsigned)R), dim3(RS_THREADS), 0,
                     as_stream(stream), src, ld_src, N_in, lens, src_rows, dst, ld_dst, N_out, dst_rows, out_lens, U, D, h, half);
  W2V2_CHECK_LAUNCH("aug_resample");
  return 0;
}
