// Scoring back-ends on the device (f32 banks, gfx950, wave64): what an LDA / PLDA evaluator needs beside score.hip.
//   w2v2_rows_center       out[r] = w_r * (x[r] - means[seg_id[r]]): the operand of a scatter matrix A^T A
//   w2v2_scatter_fold      acc (f64 [D][D]) = (first ? 0 : acc) + block (f32 [D][ldb]): the block products of a scatter
//   w2v2_plda_score_pairs  log-likelihood ratio of a trial list in the diagonalised two-covariance model
// THE DEFINITION is the "scoring back-ends" block of include/w2v2_hip.h (the project this one mirrors ships two classes
// that cannot run; the oracle is float64 numpy).  The scatter product itself is w2v2_gemm on f32 operands; the
// eigen-solves and the EM run on the host in float64.
// Conventions of the f32 strip kernels: 16-byte vectors, every guard per vector (D % 4 == 0, ld % 4 == 0), every row * ld
// in 64 bits, no atomics on global memory, no workgroup waits on another, fixed-order folds (bitwise reproducible),
// nothing allocated here, everything on the caller's stream.  The NaN and the host's row-buffer check: trial_common.h.
#include "trial_common.h"

namespace {

// ------------------------------------------------------------------------------------------ rows_center
// One row per wavefront, four per workgroup, one pass.  Per element one subtraction and one multiplication, each rounded
// to f32 on its own (nothing here can contract into an fma; the pragma says so to the compiler as well).
constexpr int RC_WAVES = 4;

__global__ __launch_bounds__(RC_WAVES * 64) void rows_center_kernel(const float* __restrict__ x, int64_t ld, int rows, int D,
                                                                    const int* __restrict__ seg_id,
                                                                    const float* __restrict__ means, int64_t ld_means, int S,
                                                                    const float* __restrict__ row_weight,
                                                                    float* __restrict__ out, int64_t ld_out) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * RC_WAVES + wave;
  if (r >= rows) return;                                    // (a whole wave; the kernel has no barrier)
  float* __restrict__ dst = out + r * ld_out;
  const int seg = seg_id ? seg_id[r] : 0;
  if (seg < 0 || seg >= S) {                                // not dereferenced: the row comes back NaN
    for (int d = lane * 4; d < D; d += 256) st4(dst + d, qnan(), qnan(), qnan(), qnan());
    return;
  }
  const float* __restrict__ row = x + r * ld;
  const float* __restrict__ mu = means + (int64_t)seg * ld_means;
  const float w = row_weight ? row_weight[r] : 1.0f;
  for (int d = lane * 4; d < D; d += 256) {
    const float4 a = ld4(row + d), m = ld4(mu + d);
    const float c0 = a.x - m.x, c1 = a.y - m.y, c2 = a.z - m.z, c3 = a.w - m.w;
    st4(dst + d, w * c0, w * c1, w * c2, w * c3);
  }
}

// ------------------------------------------------------------------------------------------ scatter_fold
// One thread per 4 consecutive elements of a row (grid-stride): one 16-byte read of the f32 block, two 16-byte reads and
// writes of the f64 accumulator.  Every element has one writer; the blocks are added in the order of the calls.
template <bool FIRST>
__global__ __launch_bounds__(256) void scatter_fold_kernel(const float* __restrict__ block, int64_t ldb,
                                                           double* __restrict__ acc, int D) {
  const int vpr = D >> 2;                                   // vectors per row
  const int64_t nv = (int64_t)D * vpr;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += (int64_t)gridDim.x * 256) {
    const int64_t i = v / vpr;
    const int j = (int)(v - i * vpr) * 4;
    const float4 b = ld4(block + i * ldb + j);
    double2* a = reinterpret_cast<double2*>(acc + i * D + j);
    double2 lo = make_double2(0.0, 0.0), hi = make_double2(0.0, 0.0);
    if constexpr (!FIRST) { lo = a[0]; hi = a[1]; }
    lo.x += (double)b.x; lo.y += (double)b.y; hi.x += (double)b.z; hi.y += (double)b.w;
    a[0] = lo;
    a[1] = hi;
  }
}

// ------------------------------------------------------------------------------------------ plda_score_pairs
// One trial per wavefront, four per workgroup, one pass over the two rows.  A lane folds the terms of its vectors in
// ascending order in double (every product is a double product of exactly converted f32 values), the 64 lane sums fold
// through the xor butterfly (the same tree in every run), k is added and the result rounds once to f32.
constexpr int PL_WAVES = 4;

__global__ __launch_bounds__(PL_WAVES * 64) void plda_score_pairs_kernel(const float* __restrict__ u, int64_t ld, int N, int Q,
                                                                         const int* __restrict__ pairs, int P,
                                                                         const double* __restrict__ pc,
                                                                         const double* __restrict__ qc, double k,
                                                                         float* __restrict__ llr_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t = (int64_t)blockIdx.x * PL_WAVES + wave;
  if (t >= P) return;                                       // (a whole wave; the kernel has no barrier)
  const int i = pairs[2 * t], j = pairs[2 * t + 1];
  if (i < 0 || i >= N || j < 0 || j >= N) {                 // not dereferenced (kept local: trial_common.h says why)
    if (lane == 0) llr_out[t] = qnan();
    return;
  }
  const float* __restrict__ re = u + (int64_t)i * ld;
  const float* __restrict__ rt = u + (int64_t)j * ld;
  double s = 0.0;
  for (int d = lane * 4; d < Q; d += 256) {
    const float4 a = ld4(re + d), b = ld4(rt + d);
    const double2 p0 = *reinterpret_cast<const double2*>(pc + d), p1 = *reinterpret_cast<const double2*>(pc + d + 2);
    const double2 q0 = *reinterpret_cast<const double2*>(qc + d), q1 = *reinterpret_cast<const double2*>(qc + d + 2);
    const double e[4] = {(double)a.x, (double)a.y, (double)a.z, (double)a.w};
    const double f[4] = {(double)b.x, (double)b.y, (double)b.z, (double)b.w};
    const double pv[4] = {p0.x, p0.y, p1.x, p1.y}, qv[4] = {q0.x, q0.y, q1.x, q1.y};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      s = fma(pv[c] * e[c], f[c], s);
      s = fma(-qv[c], fma(e[c], e[c], f[c] * f[c]), s);
    }
  }
  s = wave_sum_d(s);
  if (lane == 0) llr_out[t] = (float)(k + s);
}

}  // namespace

extern "C" int w2v2_rows_center(const float* x, int64_t ld, int rows, int D, const int32_t* seg_id, const float* means,
                                int64_t ld_means, int S, const float* row_weight, float* out, int64_t ld_out, void* stream) {
  W2V2_REQUIRE(rows_ok(x, ld, rows, D), "rows_center: bad arguments (D %% 4 == 0, ld >= D, ld %% 4 == 0, 16-byte aligned rows)");
  W2V2_REQUIRE(S >= 1 && rows_ok(means, ld_means, S, D),
               "rows_center: means is a 16-byte aligned [S][ld_means] buffer, S >= 1, ld_means >= D, ld_means %% 4 == 0");
  W2V2_REQUIRE(rows_ok(out, ld_out, rows, D) && out != x,
               "rows_center: out is a 16-byte aligned [rows][ld_out] buffer, ld_out >= D, ld_out %% 4 == 0, not the input");
  hipLaunchKernelGGL(rows_center_kernel, dim3((unsigned)cdiv(rows, RC_WAVES)), dim3(RC_WAVES * 64), 0, as_stream(stream), x, ld,
                     rows, D, seg_id, means, ld_means, S, row_weight, out, ld_out);
  W2V2_CHECK_LAUNCH("rows_center");
  return 0;
}

extern "C" int w2v2_scatter_fold(const float* block, int64_t ldb, double* acc, int D, int first, void* stream) {
  W2V2_REQUIRE(rows_ok(block, ldb, D, D) && acc && ((uintptr_t)acc & 15) == 0,
               "scatter_fold: bad arguments (D %% 4 == 0, ldb >= D, ldb %% 4 == 0, 16-byte aligned block and accumulator)");
  const dim3 grid((unsigned)blocks256((int64_t)D * (D / 4))), block_dim(256);
  if (first)
    hipLaunchKernelGGL(scatter_fold_kernel<true>, grid, block_dim, 0, as_stream(stream), block, ldb, acc, D);
  else
    hipLaunchKernelGGL(scatter_fold_kernel<false>, grid, block_dim, 0, as_stream(stream), block, ldb, acc, D);
  W2V2_CHECK_LAUNCH("scatter_fold");
  return 0;
}

extern "C" int w2v2_plda_score_pairs(const float* u, int64_t ld, int N, int Q, const int32_t* pairs, int P, const double* p,
                                     const double* q, double k, float* llr_out, void* stream) {
  W2V2_REQUIRE(rows_ok(u, ld, N, Q) && pairs && P > 0 && llr_out,
               "plda_score_pairs: bad arguments (Q %% 4 == 0, ld >= Q, ld %% 4 == 0, 16-byte aligned bank)");
  W2V2_REQUIRE(p && q && ((((uintptr_t)p) | ((uintptr_t)q)) & 15) == 0, "plda_score_pairs: p / q are 16-byte aligned [Q] doubles");
  hipLaunchKernelGGL(plda_score_pairs_kernel, dim3((unsigned)cdiv(P, PL_WAVES)), dim3(PL_WAVES * 64), 0, as_stream(stream), u, ld,
                     N, Q, pairs, P, p, q, k, llr_out);
  W2V2_CHECK_LAUNCH("plda_score_pairs");
  return 0;
}
