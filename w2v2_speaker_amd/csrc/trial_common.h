// trial_common.h -- what the trial-evaluation kernels share (score.hip: trial cosines; score_norm.hip: cohort statistics and
// normalised scores; backend.hip: LDA / PLDA; metrics.hip: sort, ROC, EER, minDCF).  Each kernel keeps its loads, its
// arithmetic and its NaN stores; the definitions that must AGREE between the stages are here, once:
//   qnan                          the quiet NaN that a trial, row or segment which cannot be evaluated comes back as
//   order_key_of / order_value_of f32 <-> u32 whose unsigned order is the order of the values: the radix sort of metrics.hip
//                                 and the top-K select of score_norm.hip tie exactly the same values
//   centre4                       the evaluator's centring of one 16-byte vector, (x - mean) / (std + 1e-12f) in f32:
//                                 score_pairs_kernel and rows_transform_kernel give an embedding the same transform
//   rows_ok                       (host) the check of an f32 row buffer: D % 4 == 0, ld >= D, ld % 4 == 0, 16-byte aligned
//   strip_common.h / common.h     StripGeom, strip_put / strip_lane_sum, ld4 / st4, wave_sum_d
// Everything here is integer work, comparisons, or f32 subtractions, additions and divisions: no product feeds a sum, so the
// header means the same in a file compiled with `#pragma clang fp contract(off)` (metrics.hip) and in one without.
// Every kernel of the five evaluation files has the instruction stream it had before these pieces were shared
// (profiles/eval_pieces_device_code.txt).  That rule keeps two pieces local:
//   the trial lookup `i = pairs[2 t], j = pairs[2 t + 1]; if (i < 0 || i >= N || j < 0 || j >= N)` of score_pairs_kernel,
//     plda_score_pairs_kernel and score_pairs_norm_kernel: every function form (indices by reference, a struct by value, the
//     NaN store as a callback) is simplified before it is inlined and tests the four bounds in one branch, where the kernels
//     branch on `i < 0` first -- 5 to 10 instructions fewer, but another stream in all three;
//   the four-wave f64 folds: block_sum_d (score_norm.hip: one sum, a barrier between butterfly and store, 4 doubles of LDS,
//     every thread reads the total) and block_fold_store / fold_rows (calibration.hip, which therefore includes nothing from
//     here: NACC sums in a [4][56] tile, one barrier, one thread per sum) share wave_sum_d (common.h) and the wave order, and
//     nothing a helper shorter than either could hold; the folds of metrics.hip are minima and integer sums.
#pragma once
#include "strip_common.h"

__device__ __forceinline__ float qnan() { return __uint_as_float(0x7fc00000u); }

// f32 bits -> u32 whose unsigned order is numpy's order of the values: -0.0 becomes +0.0 and every NaN the one largest key
// first, then the usual map (negative: all bits flipped; otherwise the sign bit set).  +inf maps to 0xff800000, the NaN key
// to 0xffffffff.  order_value_of is the inverse on the keys of numbers (the NaN key comes back as a NaN).
__device__ __forceinline__ uint32_t order_key_of(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fffffffu;
  else if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_value_of(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// center_batch of one vector of 4 features: (x - mean) / (std + 1e-12), every operation in f32
__device__ __forceinline__ float4 centre4(float4 a, const float4 m, const float4 s) {
  a.x = (a.x - m.x) / (s.x + 1e-12f); a.y = (a.y - m.y) / (s.y + 1e-12f);
  a.z = (a.z - m.z) / (s.z + 1e-12f); a.w = (a.w - m.w) / (s.w + 1e-12f);
  return a;
}

// ---------------------------------------------------------------- host side
static inline bool rows_ok(const void* p, int64_t ld, int64_t rows, int D) {
  return p && rows > 0 && D > 0 && D % 4 == 0 && ld >= D && ld % 4 == 0 && ((uintptr_t)p & 15) == 0;
}
