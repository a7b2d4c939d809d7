// strip_common.h -- what the memory-bound channels-last kernels share (tdnn.hip: BatchNorm, SE, statistics pooling;
// wav2spk.hip: InstanceNorm, gate; score.hip: embed_stats; skinny.hip: the activations; tap_gather.h: the tap gather and
// its adjoint of tdnn.hip, wav2spk.hip and conv0.hip).
// A strip is 128 columns of a [rows][C] tensor; a workgroup of 256 threads walks rows of one strip with one 16-byte vector
// per thread.  Each kernel keeps its row walk, its arithmetic and its stores; everything else is here or in common.h:
//   STRIP_CW / StripGeom<T>   the thread geometry: channels per thread, channel lanes x row lanes, rows in flight, vector types
//   strip_put / strip_lane_sum   row-lane partials -> LDS -> the sum of one channel in lane order (one sum; float or double)
//   strip_store_partial2      ... two sums per channel, all 256 threads fold, stored as a [C][2] record of a partial block
//   strip_centred_moments     block mean (double) and centred second moment of up to RPT x RL rows held in registers
//   sigmoid_f / sigmoid_bwd_f the logistic function and dy * y (1 - y) from its output
//   blocks256                 (host) workgroups of a 256-thread grid-stride launch
//   common.h                  Vec8 / Vec4f / ld4 / st4 (16-byte access), wave_sum, block_reduce_n
#pragma once
#include "common.h"
#include <type_traits>

constexpr int STRIP_CW = 128;     // channels per workgroup: 16 lanes x 8 channels, or 32 lanes x 4 f32 channels (16 B per thread)

// Thread geometry of the strip kernels.  A thread owns ONE 16-byte vector of a row: 8 channels of a 16-bit tensor, 4 of an
// f32 one -- round 6: with 8 f32 channels per thread (two 16-byte loads whose lanes sit 32 bytes apart) every load / store
// instruction used half of each 64-byte request and the f32 apply passes streamed 2.6 TB/s where a device copy of the
// same bytes streams 4.5 (profiles/r06_bn_rows_path.txt).  128 channels x RL row lanes = 256 threads either way.
template <typename T> struct StripGeom {
  static constexpr int EPT = sizeof(T) == 4 ? 4 : 8;     // channels per thread
  static constexpr int XL = STRIP_CW / EPT;              // channel lanes (blockDim.x)
  static constexpr int RL = 256 / XL;                    // row lanes (blockDim.y)
  static constexpr int UN = sizeof(T) == 4 ? 8 : 4;      // rows in flight per thread: 128 bytes either way
  using Vec = typename std::conditional<sizeof(T) == 4, Vec4f, Vec8<T>>::type;
  using FVec = typename std::conditional<sizeof(T) == 4, Vec4f, Vec8<float>>::type;   // f32 side operand, same channels
};
constexpr int STRIP_RL_MAX = 16;  // row lanes of the 16-bit geometry (8 for f32): the first extent of a shared `red`

// The fold of the row lanes' partial sums through LDS, in lane order (a fixed order: bitwise reproducible).
// strip_put: red[row lane][channel] <- the EPT sums of this thread, then the barrier; strip_lane_sum: channel c over the RL
// row lanes.  A (float or double) is the accumulator type.  `red` may be reused after the callers' next barrier.
template <int EPT, typename A, int R>
__device__ __forceinline__ void strip_put(A (&red)[R][STRIP_CW], const A* s) {
#pragma unroll
  for (int e = 0; e < EPT; ++e) red[threadIdx.y][threadIdx.x * EPT + e] = s[e];
  __syncthreads();
}
template <int RL, typename A, int R>
__device__ __forceinline__ A strip_lane_sum(A (&red)[R][STRIP_CW], int c) {
  static_assert(RL <= R, "strip_lane_sum: more row lanes than rows of red");
  A a = 0;
#pragma unroll
  for (int y = 0; y < RL; ++y) a += red[y][c];
  return a;
}
// Two sums per channel: red[row lane][channel][2] -> partial[blk][channel][2].  All 256 threads fold: thread tid takes sum
// tid >> 7 of channel tid & 127 of the strip blockIdx.x.
template <int EPT>
__device__ __forceinline__ void strip_store_partial2(float (*red)[STRIP_CW][2], const float* s1, const float* s2,
                                                     float* __restrict__ partial, int64_t blk, int C) {
  constexpr int XL = STRIP_CW / EPT, RL = 256 / XL;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    red[threadIdx.y][threadIdx.x * EPT + e][0] = s1[e];
    red[threadIdx.y][threadIdx.x * EPT + e][1] = s2[e];
  }
  __syncthreads();
  const int tid = threadIdx.y * XL + threadIdx.x;
  const int c = tid & (STRIP_CW - 1), w = tid >> 7;
  float s = 0.f;
#pragma unroll
  for (int y = 0; y < RL; ++y) s += red[y][c][w];
  const int cc = blockIdx.x * STRIP_CW + c;
  if (cc < C) partial[(blk * C + cc) * 2 + w] = s;
}

// Centred moments of a block of n <= RPT * RL rows of an f32 strip (the statistics of InstanceNorm and of embed_stats).
// This thread's vector of row t is at row0 + t * ld (`on`: the vector is inside the tensor); the rows stay in registers
// between the two passes.  The sums run in double: the mean of a constant channel is that constant exactly, and a large DC
// component costs the variance nothing (E[x^2] - mean^2 would lose mean^2 / var digits).  The squares are centred on the
// mean ROUNDED TO f32 (mu_s: x - mu_s is then an exact f32 difference for nearby x) and re-centred to the double mean:
// sum (x - m)^2 = sum (x - c)^2 - n (m - c)^2.  Threads tid < STRIP_CW return the block mean and that sum of channel tid of
// the strip and find the f32 centre in mu_s[tid]; the workgroup passes three barriers.
template <int RPT>
__device__ __forceinline__ void strip_centred_moments(const float* __restrict__ row0, int64_t ld, int n, bool on,
                                                      double (&red)[StripGeom<float>::RL][STRIP_CW], float* mu_s,
                                                      double& mean_d, double& m2) {
  using G = StripGeom<float>;
  const int cl = threadIdx.x * 4, tid = threadIdx.y * G::XL + threadIdx.x;
  float4 v[RPT];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const int t = threadIdx.y + r * G::RL;
    v[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on && t < n) v[r] = ld4(row0 + (int64_t)t * ld);
  }
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    s[0] += (double)v[r].x; s[1] += (double)v[r].y; s[2] += (double)v[r].z; s[3] += (double)v[r].w;
  }
  strip_put<4>(red, s);
  mean_d = 0.0;
  if (tid < STRIP_CW) {
    mean_d = strip_lane_sum<G::RL>(red, tid) / n;
    mu_s[tid] = (float)mean_d;                            // the centre of the squares: the mean to f32
  }
  __syncthreads();
  const float mu[4] = {mu_s[cl], mu_s[cl + 1], mu_s[cl + 2], mu_s[cl + 3]};
  double q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < RPT; ++r)
    if (threadIdx.y + r * G::RL < n) {
      const float d0 = v[r].x - mu[0], d1 = v[r].y - mu[1], d2 = v[r].z - mu[2], d3 = v[r].w - mu[3];
      q[0] += (double)d0 * d0; q[1] += (double)d1 * d1; q[2] += (double)d2 * d2; q[3] += (double)d3 * d3;
    }
  strip_put<4>(red, q);                                   // (the sums were read out of red before the barrier above)
  m2 = 0.0;
  if (tid < STRIP_CW) {
    const double off = mean_d - (double)mu_s[tid];
    m2 = fmax(strip_lane_sum<G::RL>(red, tid) - (double)n * off * off, 0.0);
  }
}

// ---------------------------------------------------------------- small activations
__device__ __forceinline__ float sigmoid_f(float v) { return 1.0f / (1.0f + __expf(-v)); }
// dy * sigmoid'(x) from the forward OUTPUT y
__device__ __forceinline__ float sigmoid_bwd_f(float dy, float y) { return dy * y * (1.0f - y); }

// ---------------------------------------------------------------- host side
// workgroups of a 256-thread grid-stride launch over n items
// (no cap below 2^20: 8192 blocks made every thread of the 60 M-element passes walk 7 strides -- the Adam kernel lost 20 % to the same cap)
static inline int blocks256(int64_t n) { const int64_t b = cdiv(n, 256); return (int)(b > (1 << 20) ? (1 << 20) : (b < 1 ? 1 : b)); }
