// Trial metrics on the device (gfx950, wave64): what follows the scores of score.hip.
//   w2v2_sort_f32_index   stable ascending argsort of P f32 keys (= np.argsort(kind="stable"): -0.0 ties with +0.0, every
//                         NaN behind +inf, ties in index order)
//   w2v2_trial_metrics    ROC (sklearn's, drop_intermediate), EER and its threshold, minDCF and its threshold of P scores
//                         and 0 / 1 labels -> eight doubles (ref: src/eval_metrics.py:54-79 and :90-206)
// No kernel waits on another workgroup: no look-back, no flag, no cooperative launch.  Every order between workgroups is a
// launch boundary (histogram | scan of the digit x tile table | scatter; block sums | scan of the sums | apply).  No
// atomics on global memory; the LDS counters are integers (any order of integer adds gives the same bits).  The output of
// the sort is unique, every step behind it is exact integer work, and the real arithmetic is f64 on those integers and on
// the f32 keys, evaluated WITHOUT contraction so that it rounds as numpy's separate operations do: equal inputs give equal
// bits.  Nothing is allocated here, everything goes on the caller's stream.  The f32 -> u32 order key of the sort is
// trial_common.h's (integer work only: it means the same above the pragma below as it would under it).
#include "trial_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SORT_THREADS = 256, SORT_WAVES = SORT_THREADS / 64, SORT_ROUNDS = 8;
constexpr int SORT_TILE = SORT_THREADS * SORT_ROUNDS;      // keys per workgroup per pass (ops.SORT_TILE)
constexpr int RADIX_BITS = 8, RADIX = 1 << RADIX_BITS, SORT_PASSES = 32 / RADIX_BITS;
constexpr int SCAN_ITEMS = 8, SCAN_TILE = 256 * SCAN_ITEMS;
constexpr int RED_TILE = 2048;                             // positions (ROC points) per workgroup of the reductions

static_assert(RADIX == SORT_THREADS, "one thread per digit loads and advances the tile's offsets");

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// ------------------------------------------------------------------------------------------ exclusive / inclusive scan
// u32 [n] in place.  (1) a workgroup scans its SCAN_TILE elements and writes its total; (2) the totals are scanned the
// same way (recursively: 2048^2 elements need two levels, 2048^3 three); (3) every workgroup adds the sum in front of it.
template <bool INCLUSIVE>
__global__ __launch_bounds__(256) void scan_block_kernel(uint32_t* __restrict__ data, int64_t n, uint32_t* __restrict__ sums) {
  __shared__ uint32_t wave_tot[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  const bool full = i0 + SCAN_ITEMS <= n;
  if (full) {                                               // (data is 16-byte aligned and i0 a multiple of 8)
    const uint4 a = *reinterpret_cast<const uint4*>(data + i0), b = *reinterpret_cast<const uint4*>(data + i0 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e) v[e] = i0 + e < n ? data[i0 + e] : 0u;
  }
  uint32_t tot = 0;
#pragma unroll
  for (int e = 0; e < SCAN_ITEMS; ++e) {                    // v[e]: the sum in front of element e (or through it)
    const uint32_t x = v[e];
    if constexpr (INCLUSIVE) { tot += x; v[e] = tot; } else { v[e] = tot; tot += x; }
  }
  uint32_t incl = tot;                                      // inclusive scan of the thread totals along the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  uint32_t pre = incl - tot;
  for (int w = 0; w < wave; ++w) pre += wave_tot[w];        // the waves in wave order
  if (full) {
    *reinterpret_cast<uint4*>(data + i0) = make_uint4(pre + v[0], pre + v[1], pre + v[2], pre + v[3]);
    *reinterpret_cast<uint4*>(data + i0 + 4) = make_uint4(pre + v[4], pre + v[5], pre + v[6], pre + v[7]);
  } else {
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e)
      if (i0 + e < n) data[i0 + e] = pre + v[e];
  }
  if (sums && threadIdx.x == 255) sums[blockIdx.x] = pre + tot;
}

__global__ __launch_bounds__(256) void scan_add_kernel(uint32_t* __restrict__ data, int64_t n, const uint32_t* __restrict__ sums) {
  const uint32_t add = sums[blockIdx.x];                    // (exclusive: the total of the workgroups in front)
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE;
#pragma unroll
  for (int e = 0; e < SCAN_ITEMS; ++e) {
    const int64_t i = i0 + e * 256 + threadIdx.x;
    if (i < n) data[i] += add;
  }
}

// u32 elements of `scratch` a scan of n elements needs (the block totals of every level, each level 16-byte aligned)
size_t scan_scratch_elems(int64_t n) {
  size_t s = 0;
  while (n > SCAN_TILE) {
    n = cdiv(n, SCAN_TILE);
    s += (size_t)((n + 3) & ~(int64_t)3);
  }
  return s;
}

int scan_u32(uint32_t* data, int64_t n, bool inclusive, uint32_t* scratch, hipStream_t st) {
  const int64_t nb = cdiv(n, SCAN_TILE);
  uint32_t* sums = nb > 1 ? scratch : nullptr;
  if (inclusive) hipLaunchKernelGGL(scan_block_kernel<true>, dim3((unsigned)nb), dim3(256), 0, st, data, n, sums);
  else hipLaunchKernelGGL(scan_block_kernel<false>, dim3((unsigned)nb), dim3(256), 0, st, data, n, sums);
  W2V2_CHECK_LAUNCH("metrics(scan)");
  if (nb == 1) return 0;
  if (scan_u32(sums, nb, false, scratch + ((nb + 3) & ~(int64_t)3), st)) return -1;
  hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)nb), dim3(256), 0, st, data, n, (const uint32_t*)sums);
  W2V2_CHECK_LAUNCH("metrics(scan add)");
  return 0;
}

// ------------------------------------------------------------------------------------------ radix sort
// The keys are order_key_of (trial_common.h) of the scores: their unsigned order is numpy's order of the values.
__global__ __launch_bounds__(256) void sort_prepare_kernel(const float* __restrict__ keys, int64_t P, uint32_t* __restrict__ ukey,
                                                           int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < P) {
    ukey[i] = order_key_of(keys[i]);
    idx[i] = (int32_t)i;
  }
}

// table[digit * ntiles + tile] = keys of the tile with that digit: scanned as one array it is, per (digit, tile), the
// number of keys with a smaller digit plus those with the same digit in the tiles in front.
__global__ __launch_bounds__(SORT_THREADS) void sort_hist_kernel(const uint32_t* __restrict__ ukey, int64_t P, int shift,
                                                                 int64_t ntiles, uint32_t* __restrict__ table) {
  __shared__ uint32_t hist[RADIX];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * SORT_TILE;
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t i = t0 + r * SORT_THREADS + threadIdx.x;
    if (i < P) atomicAdd(&hist[(ukey[i] >> shift) & (RADIX - 1)], 1u);
  }
  __syncthreads();
  table[(int64_t)threadIdx.x * ntiles + blockIdx.x] = hist[threadIdx.x];
}

// The stable scatter of one tile.  The tile goes in SORT_ROUNDS rounds of 256 consecutive keys.  In a round a lane finds
// the lanes of its wave that hold its digit (eight ballots), its rank among them (the lanes below it) and, through one LDS
// cell per (wave, digit), the keys of that digit in the waves in front of its own: destination = offset of (digit, tile)
// + keys of the digit in earlier rounds + in earlier waves + in lower lanes -- the input order, whatever the hardware's.
__global__ __launch_bounds__(SORT_THREADS) void sort_scatter_kernel(const uint32_t* __restrict__ ukey_in,
                                                                    const int32_t* __restrict__ idx_in, int64_t P, int shift,
                                                                    int64_t ntiles, const uint32_t* __restrict__ table,
                                                                    uint32_t* __restrict__ ukey_out,
                                                                    int32_t* __restrict__ idx_out) {
  __shared__ uint32_t base[RADIX];
  __shared__ uint32_t wave_cnt[SORT_WAVES][RADIX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  base[threadIdx.x] = table[(int64_t)threadIdx.x * ntiles + blockIdx.x];
#pragma unroll
  for (int w = 0; w < SORT_WAVES; ++w) wave_cnt[w][threadIdx.x] = 0;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * SORT_TILE;
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t r0 = t0 + (int64_t)r * SORT_THREADS;
    if (r0 >= P) break;                                     // (the whole workgroup)
    const int64_t i = r0 + threadIdx.x;
    const bool valid = i < P;
    const uint32_t k = valid ? ukey_in[i] : 0u;
    const int32_t v = valid ? idx_in[i] : 0;
    const uint32_t digit = (k >> shift) & (RADIX - 1);
    uint64_t same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < RADIX_BITS; ++b) {
      const bool bit = (digit >> b) & 1u;
      const uint64_t has = __ballot(valid && bit);
      same &= bit ? has : ~has;
    }
    const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wave_cnt[wave][digit] = (uint32_t)__popcll(same);
    __syncthreads();
    if (valid) {
      uint32_t dst = base[digit] + rank;
      for (int w = 0; w < wave; ++w) dst += wave_cnt[w][digit];
      if ((int64_t)dst < P) {                               // (always, for a table that was counted over these keys)
        ukey_out[dst] = k;
        idx_out[dst] = v;
      }
    }
    __syncthreads();
    uint32_t adv = 0;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) {
      adv += wave_cnt[w][threadIdx.x];
      wave_cnt[w][threadIdx.x] = 0;
    }
    base[threadIdx.x] += adv;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void sort_finish_kernel(const float* __restrict__ keys, const int32_t* __restrict__ idx, int64_t P,
                                                          int32_t* __restrict__ order_out, float* __restrict__ keys_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int32_t o = idx[i];
  if (order_out) order_out[i] = o;
  if (keys_out && o >= 0 && (int64_t)o < P) keys_out[i] = keys[o];   // the key's own bits (the sorted u32 is canonical)
}

struct SortLayout {
  int64_t ntiles, table_n;
  size_t ukey[2], idx[2], table, scratch, bytes;
};

SortLayout sort_layout(int64_t P) {
  SortLayout L;
  L.ntiles = cdiv(P, SORT_TILE);
  L.table_n = L.ntiles * RADIX;
  size_t o = 0;
  for (int s = 0; s < 2; ++s) { L.ukey[s] = o; o += align16((size_t)P * 4); }
  for (int s = 0; s < 2; ++s) { L.idx[s] = o; o += align16((size_t)P * 4); }
  L.table = o; o += align16((size_t)L.table_n * 4);
  L.scratch = o; o += align16(scan_scratch_elems(L.table_n) * 4);
  L.bytes = o;
  return L;
}

// -> the sorted canonical u32 keys and the order are left in ukey[0] / idx[0] of the workspace (four passes: back in 0)
int sort_run(const float* keys, int64_t P, int32_t* order_out, float* keys_out, char* ws, hipStream_t st) {
  const SortLayout L = sort_layout(P);
  uint32_t* uk[2] = {(uint32_t*)(ws + L.ukey[0]), (uint32_t*)(ws + L.ukey[1])};
  int32_t* ix[2] = {(int32_t*)(ws + L.idx[0]), (int32_t*)(ws + L.idx[1])};
  uint32_t* table = (uint32_t*)(ws + L.table);
  uint32_t* scratch = (uint32_t*)(ws + L.scratch);
  const dim3 flat((unsigned)cdiv(P, 256)), tiles((unsigned)L.ntiles);
  hipLaunchKernelGGL(sort_prepare_kernel, flat, dim3(256), 0, st, keys, P, uk[0], ix[0]);
  W2V2_CHECK_LAUNCH("sort_f32_index(prepare)");
  for (int pass = 0; pass < SORT_PASSES; ++pass) {
    const int s = pass & 1, shift = pass * RADIX_BITS;
    hipLaunchKernelGGL(sort_hist_kernel, tiles, dim3(SORT_THREADS), 0, st, (const uint32_t*)uk[s], P, shift, L.ntiles, table);
    W2V2_CHECK_LAUNCH("sort_f32_index(histogram)");
    if (scan_u32(table, L.table_n, false, scratch, st)) return -1;
    hipLaunchKernelGGL(sort_scatter_kernel, tiles, dim3(SORT_THREADS), 0, st, (const uint32_t*)uk[s], (const int32_t*)ix[s], P,
                       shift, L.ntiles, (const uint32_t*)table, uk[s ^ 1], ix[s ^ 1]);
    W2V2_CHECK_LAUNCH("sort_f32_index(scatter)");
  }
  static_assert(SORT_PASSES % 2 == 0, "the last pass lands in buffer 0");
  if (order_out || keys_out) {
    hipLaunchKernelGGL(sort_finish_kernel, flat, dim3(256), 0, st, keys, (const int32_t*)ix[0], P, order_out, keys_out);
    W2V2_CHECK_LAUNCH("sort_f32_index(finish)");
  }
  return 0;
}

// ------------------------------------------------------------------------------------------ trial metrics
// Over the ascending stable order: cpos[i] = positives among positions 0 .. i (inclusive scan of the gathered labels);
// gidx[i] = group ends in front of i (exclusive scan of the group-end flags), so a group end i is group gidx[i] and there
// are K = gidx[P - 1] + 1 groups.
__device__ __forceinline__ bool group_end(const uint32_t* __restrict__ ukey, int64_t i, int64_t P) {
  return i == P - 1 || ukey[i] != ukey[i + 1];
}

__global__ __launch_bounds__(256) void metrics_gather_kernel(const uint32_t* __restrict__ ukey, const int32_t* __restrict__ order,
                                                             const uint8_t* __restrict__ labels, int64_t P,
                                                             uint32_t* __restrict__ cpos, uint32_t* __restrict__ gidx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const uint32_t o = (uint32_t)order[i];                    // (a permutation of 0 .. P - 1; never trusted as an address)
  cpos[i] = (int64_t)o < P && labels[o] != 0 ? 1u : 0u;
  gidx[i] = group_end(ukey, i, P) ? 1u : 0u;
}

// the group ends, dense and ascending: e_pos[g] = position of the end of group g, e_cp[g] = cpos there
__global__ __launch_bounds__(256) void metrics_compact_kernel(const uint32_t* __restrict__ ukey, const uint32_t* __restrict__ cpos,
                                                              const uint32_t* __restrict__ gidx, int64_t P,
                                                              uint32_t* __restrict__ e_pos, uint32_t* __restrict__ e_cp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P || !group_end(ukey, i, P)) return;
  const uint32_t g = gidx[i];                               // < K <= P
  e_pos[g] = (uint32_t)i;
  e_cp[g] = cpos[i];
}

// minDCF, eval_metrics.calculate_mdc: c_det at EVERY position of the stable order, the lowest index among equal minima
struct MinAt { double v; int32_t i; int32_t pad; };

__device__ __forceinline__ bool min_before(double v, int32_t i, double ov, int32_t oi) {
  return v < ov || (v == ov && i < oi);
}
__device__ __forceinline__ void min_fold_wave(double& v, int32_t& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int32_t oi = __shfl_xor(i, o, 64);
    if (min_before(ov, oi, v, i)) { v = ov; i = oi; }
  }
}
// (value, index) minimum of a workgroup of four waves -> valid in thread 0; the minimum with the lowest index is the same
// whatever the order of the comparisons (nothing is rounded)
__device__ __forceinline__ void min_fold_block(double& v, int32_t& i, double* sv, int32_t* si) {
  min_fold_wave(v, i);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sv[wave] = v; si[wave] = i; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w)
      if (min_before(sv[w], si[w], v, i)) { v = sv[w]; i = si[w]; }
}

constexpr int32_t NO_INDEX = 0x7fffffff;

__global__ __launch_bounds__(256) void metrics_mdc_kernel(const uint32_t* __restrict__ cpos, int64_t P, double c_miss, double c_fa,
                                                          double p_target, MinAt* __restrict__ partial) {
  __shared__ double sv[4];
  __shared__ int32_t si[4];
  const double n_pos = (double)cpos[P - 1], n_neg = (double)P - n_pos, q_target = 1.0 - p_target;
  double best = INFINITY;
  int32_t at = NO_INDEX;
  const int64_t i0 = (int64_t)blockIdx.x * RED_TILE;
#pragma unroll 2
  for (int r = 0; r < RED_TILE / 256; ++r) {
    const int64_t i = i0 + r * 256 + threadIdx.x;
    if (i < P) {
      const double cp = (double)cpos[i], cn = (double)(i + 1) - cp;
      const double fnr = cp / n_pos, fpr = 1.0 - cn / n_neg;
      const double c_det = __dadd_rn(__dmul_rn(__dmul_rn(c_miss, fnr), p_target), __dmul_rn(__dmul_rn(c_fa, fpr), q_target));
      if (min_before(c_det, (int32_t)i, best, at)) { best = c_det; at = (int32_t)i; }
    }
  }
  min_fold_block(best, at, sv, si);
  if (threadIdx.x == 0) { partial[blockIdx.x].v = best; partial[blockIdx.x].i = at; partial[blockIdx.x].pad = 0; }
}

// The ROC, sklearn's: point 0 is the origin, point j = 1 .. K the group ends in DESCENDING score order (group g = K - j),
// tp / fp = the positives / negatives at or above that score = everything behind the end of the group in front.
struct Roc {
  const uint32_t *e_pos, *e_cp;
  int64_t K, n_pos, n_neg;
};
__device__ __forceinline__ void roc_point(const Roc& r, int64_t j, int64_t& tp, int64_t& fp) {
  const int64_t g = r.K - j;
  if (j <= 0) { tp = 0; fp = 0; return; }
  if (g <= 0) { tp = r.n_pos; fp = r.n_neg; return; }
  const int64_t cp = r.e_cp[g - 1], pos = r.e_pos[g - 1];
  tp = r.n_pos - cp;
  fp = r.n_neg - (pos + 1 - cp);
}
// 1 - fp / N - tp / Pn <= 0, exactly
__device__ __forceinline__ bool roc_passes(const Roc& r, int64_t tp, int64_t fp) {
  return fp * r.n_pos + tp * r.n_neg >= r.n_neg * r.n_pos;
}

// Kept points (drop_intermediate): the origin, the first and the last point always; a point between them iff the second
// difference of fp or of tp is non-zero there.  hi = the first kept point that passes, lo = the last kept point that does
// not; both are index reductions, a collinear run is never walked.
struct RocPartial { int32_t hi, lo, kept, pad; };

__global__ __launch_bounds__(256) void metrics_roc_kernel(const uint32_t* __restrict__ cpos, const uint32_t* __restrict__ gidx,
                                                          const uint32_t* __restrict__ e_pos, const uint32_t* __restrict__ e_cp,
                                                          int64_t P, RocPartial* __restrict__ partial) {
  __shared__ int32_t s_hi[4], s_lo[4], s_kept[4];
  Roc roc;
  roc.e_pos = e_pos; roc.e_cp = e_cp;
  roc.K = (int64_t)gidx[P - 1] + 1;
  roc.n_pos = cpos[P - 1];
  roc.n_neg = P - roc.n_pos;
  int32_t hi = NO_INDEX, lo = -1, kept = 0;
  const int64_t j0 = (int64_t)blockIdx.x * RED_TILE;
  for (int r = 0; r < RED_TILE / 256; ++r) {
    const int64_t j = j0 + r * 256 + threadIdx.x;
    if (j > roc.K) continue;
    int64_t tp, fp;
    roc_point(roc, j, tp, fp);
    bool keep = j <= 1 || j == roc.K;
    if (!keep) {
      int64_t tpa, fpa, tpb, fpb;
      roc_point(roc, j - 1, tpa, fpa);
      roc_point(roc, j + 1, tpb, fpb);
      keep = (fpa - 2 * fp + fpb) != 0 || (tpa - 2 * tp + tpb) != 0;
    }
    if (!keep) continue;
    ++kept;
    if (roc_passes(roc, tp, fp)) hi = min(hi, (int32_t)j);
    else lo = max(lo, (int32_t)j);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hi = min(hi, __shfl_xor(hi, o, 64));
    lo = max(lo, __shfl_xor(lo, o, 64));
    kept += __shfl_xor(kept, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_hi[wave] = hi; s_lo[wave] = lo; s_kept[wave] = kept; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) { hi = min(hi, s_hi[w]); lo = max(lo, s_lo[w]); kept += s_kept[w]; }
    partial[blockIdx.x] = RocPartial{hi, lo, kept, 0};
  }
}

// One workgroup folds the partials; its first thread finishes the closed forms in f64.
__global__ __launch_bounds__(256) void metrics_finish_kernel(const float* __restrict__ skeys, const uint32_t* __restrict__ cpos,
                                                             const uint32_t* __restrict__ gidx, const uint32_t* __restrict__ e_pos,
                                                             const uint32_t* __restrict__ e_cp, int64_t P,
                                                             const MinAt* __restrict__ mdc_partial, int64_t n_mdc,
                                                             const RocPartial* __restrict__ roc_partial, int64_t n_roc,
                                                             double c_miss, double c_fa, double p_target, double* __restrict__ out) {
  __shared__ double sv[4];
  __shared__ int32_t si[4];
  __shared__ int32_t s_hi[4], s_lo[4];
  __shared__ long long s_kept[4];
  double best = INFINITY;
  int32_t at = NO_INDEX;
  for (int64_t b = threadIdx.x; b < n_mdc; b += 256)
    if (min_before(mdc_partial[b].v, mdc_partial[b].i, best, at)) { best = mdc_partial[b].v; at = mdc_partial[b].i; }
  min_fold_block(best, at, sv, si);
  int32_t hi = NO_INDEX, lo = -1;
  long long kept = 0;
  for (int64_t b = threadIdx.x; b < n_roc; b += 256) {
    hi = min(hi, roc_partial[b].hi);
    lo = max(lo, roc_partial[b].lo);
    kept += roc_partial[b].kept;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hi = min(hi, __shfl_xor(hi, o, 64));
    lo = max(lo, __shfl_xor(lo, o, 64));
    kept += __shfl_xor(kept, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_hi[wave] = hi; s_lo[wave] = lo; s_kept[wave] = kept; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < 4; ++w) { hi = min(hi, s_hi[w]); lo = max(lo, s_lo[w]); kept += s_kept[w]; }

  Roc roc;
  roc.e_pos = e_pos; roc.e_cp = e_cp;
  roc.K = (int64_t)gidx[P - 1] + 1;
  roc.n_pos = cpos[P - 1];
  roc.n_neg = P - roc.n_pos;
  const double N = (double)roc.n_neg, Pn = (double)roc.n_pos, nan = __longlong_as_double(0x7ff8000000000000ll);
  // NaN scores are the tail of the order: the first of them by bisection
  int64_t a = 0, b = P;
  while (a < b) {
    const int64_t m = a + (b - a) / 2;
    if (isnan(skeys[m])) b = m; else a = m + 1;
  }
  double eer = nan, eer_thr = nan;
  if (lo >= 0 && (int64_t)hi <= roc.K && lo < hi) {         // (a list of one class has no point on one of the sides)
    int64_t tp0, fp0, tp1, fp1;
    roc_point(roc, lo, tp0, fp0);
    roc_point(roc, hi, tp1, fp1);
    const double thr1 = (double)skeys[min((int64_t)e_pos[roc.K - hi], P - 1)];   // (a position: < P)
    if (fp0 == fp1) {                                       // a vertical segment
      eer = (double)fp1 / N;
      eer_thr = thr1;
    } else {
      const double x0 = (double)fp0 / N, x1 = (double)fp1 / N, y0 = (double)tp0 / Pn, y1 = (double)tp1 / Pn;
      const double m = (y1 - y0) / (x1 - x0);
      eer = (1.0 - y0 + m * x0) / (1.0 + m);
      if (lo > 0) {
        const double thr0 = (double)skeys[min((int64_t)e_pos[roc.K - lo], P - 1)];
        eer_thr = thr0 + (eer - x0) * (thr1 - thr0) / (x1 - x0);
      }
    }
    if (lo == 0) eer_thr = INFINITY;                        // the origin's threshold
  }
  double mdc = nan, mdc_thr = nan;
  if (at != NO_INDEX) {
    const double c_def = fmin(c_miss * p_target, c_fa * (1.0 - p_target));
    mdc = best / c_def;
    mdc_thr = (double)skeys[at];
  }
  out[0] = eer; out[1] = eer_thr; out[2] = mdc; out[3] = mdc_thr;
  out[4] = Pn; out[5] = N; out[6] = (double)(P - a); out[7] = (double)kept;
}

struct MetricsLayout {
  size_t sort, order, skeys, cpos, gidx, e_pos, e_cp, scratch, mdc_partial, roc_partial, bytes;
  int64_t n_mdc, n_roc;
};

MetricsLayout metrics_layout(int64_t P) {
  MetricsLayout L;
  size_t o = 0;
  L.sort = o; o += sort_layout(P).bytes;
  size_t* const arrays[] = {&L.order, &L.skeys, &L.cpos, &L.gidx, &L.e_pos, &L.e_cp};
  for (size_t* a : arrays) { *a = o; o += align16((size_t)P * 4); }
  L.scratch = o; o += align16(scan_scratch_elems(P) * 4);
  L.n_mdc = cdiv(P, RED_TILE);
  L.n_roc = cdiv(P + 1, RED_TILE);
  L.mdc_partial = o; o += (size_t)L.n_mdc * sizeof(MinAt);
  L.roc_partial = o; o += (size_t)L.n_roc * sizeof(RocPartial);
  L.bytes = o;
  return L;
}

static_assert(sizeof(MinAt) == 16 && sizeof(RocPartial) == 16, "the partials keep the layout 16-byte aligned");

bool count_ok(int64_t P) { return P >= 1 && P <= 0x7fffffffll; }

}  // namespace

extern "C" int w2v2_sort_tile(void) { return SORT_TILE; }

extern "C" int64_t w2v2_sort_f32_index_workspace_bytes(int64_t P) {
  return count_ok(P) ? (int64_t)sort_layout(P).bytes : -1;
}

extern "C" int w2v2_sort_f32_index(const float* keys, int64_t P, int32_t* order_out, float* keys_out, void* workspace,
                                   void* stream) {
  W2V2_REQUIRE(count_ok(P), "sort_f32_index: P = %lld outside [1, 2^31)", (long long)P);
  W2V2_REQUIRE(keys && order_out && workspace && ((uintptr_t)workspace & 15) == 0,
               "sort_f32_index: bad arguments (keys, order_out and a 16-byte aligned workspace are required)");
  return sort_run(keys, P, order_out, keys_out, (char*)workspace, as_stream(stream));
}

extern "C" int64_t w2v2_trial_metrics_workspace_bytes(int64_t P) {
  return count_ok(P) ? (int64_t)metrics_layout(P).bytes : -1;
}

extern "C" int w2v2_trial_metrics(const float* scores, const uint8_t* labels, int64_t P, double c_miss, double c_fa,
                                  double p_target, double* out, void* workspace, void* stream) {
  W2V2_REQUIRE(count_ok(P), "trial_metrics: P = %lld outside [1, 2^31)", (long long)P);
  W2V2_REQUIRE(scores && labels && out && workspace && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out & 7) == 0,
               "trial_metrics: bad arguments (scores, labels, an 8-byte aligned out[8] and a 16-byte aligned workspace)");
  W2V2_REQUIRE(c_miss >= 1.0 && c_fa >= 1.0 && p_target >= 0.0 && p_target <= 1.0,
               "trial_metrics: c_miss >= 1, c_fa >= 1 and 0 <= p_target <= 1 (calculate_mdc's own conditions)");
  hipStream_t st = as_stream(stream);
  char* ws = (char*)workspace;
  const MetricsLayout L = metrics_layout(P);
  const SortLayout S = sort_layout(P);
  int32_t* order = (int32_t*)(ws + L.order);
  float* skeys = (float*)(ws + L.skeys);
  uint32_t *cpos = (uint32_t*)(ws + L.cpos), *gidx = (uint32_t*)(ws + L.gidx);
  uint32_t *e_pos = (uint32_t*)(ws + L.e_pos), *e_cp = (uint32_t*)(ws + L.e_cp);
  uint32_t* scratch = (uint32_t*)(ws + L.scratch);
  MinAt* mdc_partial = (MinAt*)(ws + L.mdc_partial);
  RocPartial* roc_partial = (RocPartial*)(ws + L.roc_partial);
  if (sort_run(scores, P, order, skeys, ws + L.sort, st)) return -1;
  const uint32_t* ukey = (const uint32_t*)(ws + L.sort + S.ukey[0]);
  const dim3 flat((unsigned)cdiv(P, 256));
  hipLaunchKernelGGL(metrics_gather_kernel, flat, dim3(256), 0, st, ukey, (const int32_t*)order, labels, P, cpos, gidx);
  W2V2_CHECK_LAUNCH("trial_metrics(gather)");
  if (scan_u32(cpos, P, true, scratch, st) || scan_u32(gidx, P, false, scratch, st)) return -1;
  hipLaunchKernelGGL(metrics_compact_kernel, flat, dim3(256), 0, st, ukey, (const uint32_t*)cpos, (const uint32_t*)gidx, P, e_pos,
                     e_cp);
  W2V2_CHECK_LAUNCH("trial_metrics(compact)");
  hipLaunchKernelGGL(metrics_mdc_kernel, dim3((unsigned)L.n_mdc), dim3(256), 0, st, (const uint32_t*)cpos, P, c_miss, c_fa,
                     p_target, mdc_partial);
  W2V2_CHECK_LAUNCH("trial_metrics(minDCF)");
  hipLaunchKernelGGL(metrics_roc_kernel, dim3((unsigned)L.n_roc), dim3(256), 0, st, (const uint32_t*)cpos, (const uint32_t*)gidx,
                     (const uint32_t*)e_pos, (const uint32_t*)e_cp, P, roc_partial);
  W2V2_CHECK_LAUNCH("trial_metrics(ROC)");
  hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)skeys, (const uint32_t*)cpos,
                     (const uint32_t*)gidx, (const uint32_t*)e_pos, (const uint32_t*)e_cp, P, (const MinAt*)mdc_partial, L.n_mdc,
                     (const RocPartial*)roc_partial, L.n_roc, c_miss, c_fa, p_target, out);
  W2V2_CHECK_LAUNCH("trial_metrics(finish)");
  return 0;
}
