// Score calibration and fusion on the device (gfx950, wave64): what turns the trial scores of score.hip / score_norm.hip /
// backend.hip into log-likelihood ratios, and what says how good they are as such.
//   w2v2_calib_fit     prior-weighted logistic regression of K systems' scores -> an f64 state record on the device
//   w2v2_calib_apply   llr = a_0 + sum_k a_k s_k with the affine map read from the record
//   w2v2_llr_metrics   Cllr and actDCF at the Bayes threshold -> eight doubles
// The definition is the "score calibration" block of include/w2v2_hip.h.  The conventions are those of metrics.hip: no
// kernel waits on another workgroup, every order between workgroups is a launch boundary, no atomics on global memory,
// per-workgroup partials go to the caller's workspace and are folded in ascending order by one workgroup.  Every sum and
// every transcendental is f64, evaluated WITHOUT contraction; every fold has a fixed order: equal inputs give equal bits.
// The whole fit is enqueued at once: a round's statistics kernel reads the status from the record and returns when the
// fit has ended, so the host never waits between rounds.  Nothing is allocated here, everything goes on the caller's stream.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CAL_THREADS = 256, CAL_WAVES = CAL_THREADS / 64, CAL_GROUPS = 2;
constexpr int CAL_TILE = CAL_THREADS * 4 * CAL_GROUPS;     // trials per workgroup (ops.CALIB_TILE): 2 x 4 a thread
constexpr int MAXK = W2V2_CALIB_MAX_SYSTEMS, MAXN = MAXK + 1;
constexpr int MAX_ACC = 1 + MAXN + MAXN * (MAXN + 1) / 2;  // J, g, the upper triangle of H: 55 doubles at K = 8
constexpr int PART_LD = 56;                                // doubles per workgroup row of the workspace
static_assert(MAX_ACC <= PART_LD && PART_LD <= CAL_THREADS, "one thread per folded element");

// the f64 state record (w2v2_calib_record_doubles() doubles; the layout is part of the header's definition)
enum : int {
  R_STATUS = 0, R_ROUNDS = 1, R_K = 2, R_J = 3, R_STEP = 4, R_DEC = 5, R_NTAR = 6, R_NNON = 7, R_NNAN = 8, R_JTRIAL = 9,
  R_W = 16, R_D = R_W + MAXN, R_WT = R_D + MAXN, R_MEAN = R_WT + MAXN, R_SD = R_MEAN + MAXK, R_RINV = R_SD + MAXK,
  R_A = R_RINV + MAXK, R_G = R_A + MAXN, R_H = R_G + MAXN, R_DOUBLES = 168
};
static_assert(R_H + MAXN * MAXN <= R_DOUBLES, "the record holds H whole");

constexpr double ST_RUNNING = 0.0, ST_CONVERGED = 1.0, ST_FAILED = 2.0, ST_SMALL_STEP = 3.0;
constexpr double DEC_STOP = 1e-12, STEP_MIN = 1.0 / 1048576.0;      // 2^-20

struct Start { double w[MAXN]; int given; int pad; };

inline bool count_ok(int64_t P) { return P >= 1 && P <= 0x7fffffffll; }
inline int64_t tiles_of(int64_t P) { return cdiv(P, CAL_TILE); }

// The trials of this workgroup's tile that belong to this thread, in ascending order: two groups of four consecutive
// trials.  `vec`: every row of S is 16-byte aligned (ld % 4 == 0) and the labels 4-byte aligned, so a whole group is one
// 16-byte load per system and one 4-byte load of labels; the last, short group and unaligned inputs take scalar loads.
// Nothing at or behind index P is read (a row's pad may hold anything).
template <int K, typename F>
__device__ __forceinline__ void tile_trials(const float* __restrict__ S, int64_t ld, const uint8_t* __restrict__ labels, int64_t P,
                                            bool vec, F&& f) {
  const int64_t t0 = (int64_t)blockIdx.x * CAL_TILE;
#pragma unroll
  for (int h = 0; h < CAL_GROUPS; ++h) {
    const int64_t i0 = t0 + h * (CAL_THREADS * 4) + threadIdx.x * 4;
    if (i0 >= P) continue;
    const int n = P - i0 < 4 ? (int)(P - i0) : 4;
    float s[4][K];
    bool y[4] = {false, false, false, false};
    if (vec && n == 4) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float4 v = ld4(S + (int64_t)k * ld + i0);
        s[0][k] = v.x; s[1][k] = v.y; s[2][k] = v.z; s[3][k] = v.w;
      }
      const uint32_t yy = *reinterpret_cast<const uint32_t*>(labels + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = ((yy >> (8 * e)) & 0xffu) != 0;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int k = 0; k < K; ++k) s[e][k] = e < n ? S[(int64_t)k * ld + i0 + e] : 0.0f;
        y[e] = e < n ? labels[i0 + e] != 0 : false;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < n) f(s[e], y[e]);
  }
}

// NACC per-thread sums -> one row of the workspace: the xor butterfly of a wave (a + b and b + a are the same double, so
// every lane holds the same bits), then the four waves in wave order.
template <int NACC>
__device__ __forceinline__ void block_fold_store(double (&acc)[NACC], double* __restrict__ row) {
  __shared__ double sh[CAL_WAVES][PART_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < NACC; ++a) {
    const double v = wave_sum_d(acc[a]);
    if (lane == 0) sh[wave][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < NACC) {
    double v = sh[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < CAL_WAVES; ++w) v += sh[w][threadIdx.x];
    row[threadIdx.x] = v;
  }
}

// nacc columns of nblk workspace rows, each summed by one thread in ascending row order -> out[0 .. nacc) in LDS
__device__ __forceinline__ void fold_rows(const double* __restrict__ partial, int64_t nblk, int nacc, double* out) {
  if ((int)threadIdx.x < nacc) {
    double v = 0.0;
    for (int64_t b = 0; b < nblk; ++b) v += partial[b * PART_LD + threadIdx.x];
    out[threadIdx.x] = v;
  }
  __syncthreads();
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// ------------------------------------------------------------------------------------------ step 1: the moments
// pass 1: sum_k, targets, NaN trials (a trial with a NaN in any system)
template <int K>
__global__ __launch_bounds__(CAL_THREADS) void calib_sum_kernel(const float* __restrict__ S, int64_t ld, const uint8_t* __restrict__ labels,
                                                                int64_t P, int vec, double* __restrict__ partial) {
  double acc[K + 2];
#pragma unroll
  for (int a = 0; a < K + 2; ++a) acc[a] = 0.0;
  tile_trials<K>(S, ld, labels, P, vec != 0, [&](const float (&s)[K], bool y) {
    bool nan = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      acc[k] += (double)s[k];
      nan = nan || s[k] != s[k];
    }
    acc[K] += y ? 1.0 : 0.0;
    acc[K + 1] += nan ? 1.0 : 0.0;
  });
  block_fold_store<K + 2>(acc, partial + (int64_t)blockIdx.x * PART_LD);
}

// ... folded: the record is written whole here (whatever the caller's buffer held), means and counts set
__global__ __launch_bounds__(CAL_THREADS) void calib_mean_kernel(const double* __restrict__ partial, int64_t nblk, int K, int64_t P,
                                                                 double* __restrict__ rec) {
  __shared__ double tot[PART_LD];
  __shared__ double init[R_DOUBLES];
  fold_rows(partial, nblk, K + 2, tot);
  if (threadIdx.x < R_DOUBLES) init[threadIdx.x] = 0.0;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 0; k < K; ++k) init[R_MEAN + k] = tot[k] / (double)P;
    const double n_tar = tot[K], n_nan = tot[K + 1];
    init[R_K] = (double)K;
    init[R_NTAR] = n_tar;
    init[R_NNON] = (double)P - n_tar;
    init[R_NNAN] = n_nan;
    init[R_STATUS] = (n_nan > 0.0 || n_tar == 0.0 || n_tar == (double)P) ? ST_FAILED : ST_RUNNING;
  }
  __syncthreads();
  if (threadIdx.x < R_DOUBLES) rec[threadIdx.x] = init[threadIdx.x];      // one writer per cell
}
static_assert(R_DOUBLES <= CAL_THREADS, "one thread per cell clears the record");

// pass 2: sum (s - m_k)^2
template <int K>
__global__ __launch_bounds__(CAL_THREADS) void calib_dev_kernel(const float* __restrict__ S, int64_t ld, const uint8_t* __restrict__ labels,
                                                                int64_t P, int vec, const double* __restrict__ rec,
                                                                double* __restrict__ partial) {
  if (rec[R_STATUS] != ST_RUNNING) return;
  double m[K], acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { m[k] = rec[R_MEAN + k]; acc[k] = 0.0; }
  tile_trials<K>(S, ld, labels, P, vec != 0, [&](const float (&s)[K], bool) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double d = (double)s[k] - m[k];
      acc[k] += d * d;
    }
  });
  block_fold_store<K>(acc, partial + (int64_t)blockIdx.x * PART_LD);
}

__global__ __launch_bounds__(CAL_THREADS) void calib_std_kernel(const double* __restrict__ partial, int64_t nblk, int K, int64_t P,
                                                                Start start, double* __restrict__ rec) {
  __shared__ double tot[PART_LD];
  if (rec[R_STATUS] != ST_RUNNING) return;
  fold_rows(partial, nblk, K, tot);
  if (threadIdx.x != 0) return;
  bool ok = true;
  for (int k = 0; k < K; ++k) {
    const double sd = sqrt(tot[k] / (double)(P - 1));
    rec[R_SD + k] = sd;
    rec[R_RINV + k] = 1.0 / sd;
    ok = ok && sd > 0.0 && finite_d(sd) && finite_d(1.0 / sd);
  }
  for (int a = 0; a <= K; ++a) {
    const double w = start.given ? start.w[a] : 0.0;
    rec[R_W + a] = w;
    rec[R_WT + a] = w;
  }
  rec[R_STEP] = 1.0;
  rec[R_J] = INFINITY;
  if (!ok) rec[R_STATUS] = ST_FAILED;
}

// ------------------------------------------------------------------------------------------ step 2: J, g, H at the trial point
// sigma(z) and sigma(-z) from one exponential, each as a quotient that cannot overflow; softplus(a) = max(a, 0) +
// log1p(exp(-|a|)) with |a| = |z| for either class.
template <int K>
__global__ __launch_bounds__(CAL_THREADS) void calib_stats_kernel(const float* __restrict__ S, int64_t ld, const uint8_t* __restrict__ labels,
                                                                  int64_t P, int vec, double pi, double tau,
                                                                  const double* __restrict__ rec, double* __restrict__ partial) {
  if (rec[R_STATUS] != ST_RUNNING) return;
  constexpr int N = K + 1, NACC = 1 + N + N * (N + 1) / 2;
  double w[N], m[K], r[K], acc[NACC];
#pragma unroll
  for (int a = 0; a < N; ++a) w[a] = rec[R_WT + a];
#pragma unroll
  for (int k = 0; k < K; ++k) { m[k] = rec[R_MEAN + k]; r[k] = rec[R_RINV + k]; }
  const double c_tar = pi / rec[R_NTAR], c_non = (1.0 - pi) / rec[R_NNON];
#pragma unroll
  for (int a = 0; a < NACC; ++a) acc[a] = 0.0;
  tile_trials<K>(S, ld, labels, P, vec != 0, [&](const float (&s)[K], bool y) {
    double x[N];
    x[0] = 1.0;
    double l = w[0];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      x[k + 1] = ((double)s[k] - m[k]) * r[k];
      l = l + w[k + 1] * x[k + 1];
    }
    const double z = l + tau;
    const double e = exp(-fabs(z)), lp = log1p(e), inv = 1.0 / (1.0 + e);
    const double big = inv, small = e * inv;               // sigma(|z|), sigma(-|z|)
    const double p = z >= 0.0 ? big : small, q = z >= 0.0 ? small : big;
    const double c = y ? c_tar : c_non;
    acc[0] += c * (fmax(y ? -z : z, 0.0) + lp);
    const double gc = c * (y ? -q : p), hc = c * (p * q);
#pragma unroll
    for (int a = 0; a < N; ++a) acc[1 + a] += gc * x[a];
    int at = 1 + N;
#pragma unroll
    for (int a = 0; a < N; ++a) {
      const double ha = hc * x[a];
#pragma unroll
      for (int b = a; b < N; ++b) acc[at++] += ha * x[b];
    }
  });
  block_fold_store<NACC>(acc, partial + (int64_t)blockIdx.x * PART_LD);
}

// ------------------------------------------------------------------------------------------ step 3: fold, Newton, step halving
__device__ void affine_map(double* rec, int K) {
  double a0 = rec[R_W];
  for (int k = 0; k < K; ++k) {
    const double ak = rec[R_W + 1 + k] * rec[R_RINV + k];
    rec[R_A + 1 + k] = ak;
    a0 = a0 - ak * rec[R_MEAN + k];
  }
  rec[R_A] = a0;
}

// A decrement below the stop value at a point where J < min(c_tar, c_non) ln 2 is NOT convergence when ridge = 0: a trial on
// the wrong side of its own threshold costs at least c_i ln 2, so such a J proves that every trial lies on its right side --
// the set is separable, J has no minimum and only falls towards 0 (by about a factor e per round).  The fit then keeps
// running and ends as "not converged after max_iter".
__global__ __launch_bounds__(CAL_THREADS) void calib_solve_kernel(const double* __restrict__ partial, int64_t nblk, int K, double ridge,
                                                                  double pi, double* __restrict__ rec) {
  __shared__ double tot[PART_LD];
  __shared__ double g[MAXN], H[MAXN][MAXN], L[MAXN][MAXN], d[MAXN], wt[MAXN];
  if (rec[R_STATUS] != ST_RUNNING) return;
  const int N = K + 1;
  fold_rows(partial, nblk, 1 + N + N * (N + 1) / 2, tot);
  if (threadIdx.x != 0) return;
  double J = tot[0], pen = 0.0;
  bool ok = true;
  for (int a = 0; a < N; ++a) wt[a] = rec[R_WT + a];
  for (int a = 1; a < N; ++a) pen += wt[a] * wt[a];
  J = J + (ridge * 0.5) * pen;
  for (int a = 0; a < N; ++a) g[a] = tot[1 + a] + (a > 0 ? ridge * wt[a] : 0.0);
  int at = 1 + N;
  for (int a = 0; a < N; ++a)
    for (int b = a; b < N; ++b) {
      const double v = tot[at++] + (a == b && a > 0 ? ridge : 0.0);
      H[a][b] = v;
      H[b][a] = v;
      ok = ok && finite_d(v);
    }
  ok = ok && finite_d(J);
  for (int a = 0; a < N; ++a) ok = ok && finite_d(g[a]);
  const double rounds = rec[R_ROUNDS] + 1.0;
  rec[R_ROUNDS] = rounds;
  rec[R_JTRIAL] = J;
  if (!ok) { rec[R_STATUS] = ST_FAILED; return; }
  if (rounds > 1.0 && J > rec[R_J]) {                       // rejected: halve the step along the kept direction
    const double step = rec[R_STEP] * 0.5;
    rec[R_STEP] = step;
    if (step < STEP_MIN) { rec[R_STATUS] = ST_SMALL_STEP; return; }
    for (int a = 0; a < N; ++a) rec[R_WT + a] = rec[R_W + a] - step * rec[R_D + a];
    return;
  }
  rec[R_J] = J;                                             // accepted
  for (int a = 0; a < N; ++a) {
    rec[R_W + a] = wt[a];
    rec[R_G + a] = g[a];
    for (int b = 0; b < N; ++b) rec[R_H + a * MAXN + b] = H[a][b];
  }
  affine_map(rec, K);
  for (int j = 0; j < N; ++j) {                             // H = L L^T
    double s = H[j][j];
    for (int c = 0; c < j; ++c) s = s - L[j][c] * L[j][c];
    if (!(s > 0.0) || !finite_d(s)) { rec[R_STATUS] = ST_FAILED; return; }
    const double ljj = sqrt(s);
    L[j][j] = ljj;
    for (int i = j + 1; i < N; ++i) {
      double t = H[i][j];
      for (int c = 0; c < j; ++c) t = t - L[i][c] * L[j][c];
      L[i][j] = t / ljj;
    }
  }
  for (int i = 0; i < N; ++i) {                             // L y = g
    double t = g[i];
    for (int c = 0; c < i; ++c) t = t - L[i][c] * d[c];
    d[i] = t / L[i][i];
  }
  for (int i = N - 1; i >= 0; --i) {                        // L^T d = y
    double t = d[i];
    for (int c = i + 1; c < N; ++c) t = t - L[c][i] * d[c];
    d[i] = t / L[i][i];
  }
  double dec = 0.0;
  for (int a = 0; a < N; ++a) dec = dec + g[a] * d[a];
  dec = dec * 0.5;
  rec[R_DEC] = dec;
  if (!finite_d(dec)) { rec[R_STATUS] = ST_FAILED; return; }
  for (int a = 0; a < N; ++a) rec[R_D + a] = d[a];
  const double c_min = fmin(pi / rec[R_NTAR], (1.0 - pi) / rec[R_NNON]);
  const bool separated = ridge == 0.0 && J < c_min * 0.6931471805599453;
  if (dec < DEC_STOP && !separated) { rec[R_STATUS] = ST_CONVERGED; return; }
  rec[R_STEP] = 1.0;
  for (int a = 0; a < N; ++a) rec[R_WT + a] = wt[a] - d[a];
}

// ------------------------------------------------------------------------------------------ step 5: apply
template <int K>
__global__ __launch_bounds__(CAL_THREADS) void calib_apply_kernel(const float* __restrict__ S, int64_t ld, int64_t P, int vec,
                                                                  const double* __restrict__ a, float* __restrict__ out) {
  double c[K + 1];
#pragma unroll
  for (int k = 0; k <= K; ++k) c[k] = a[k];
  const int64_t i0 = ((int64_t)blockIdx.x * CAL_THREADS + threadIdx.x) * 4;
  if (i0 >= P) return;
  const int n = P - i0 < 4 ? (int)(P - i0) : 4;
  double l[4] = {c[0], c[0], c[0], c[0]};
  if (vec && n == 4) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float4 v = ld4(S + (int64_t)k * ld + i0);
      l[0] = l[0] + c[k + 1] * (double)v.x;
      l[1] = l[1] + c[k + 1] * (double)v.y;
      l[2] = l[2] + c[k + 1] * (double)v.z;
      l[3] = l[3] + c[k + 1] * (double)v.w;
    }
    *reinterpret_cast<float4*>(out + i0) = make_float4((float)l[0], (float)l[1], (float)l[2], (float)l[3]);
    return;
  }
  for (int e = 0; e < n; ++e) {
    double v = c[0];
#pragma unroll
    for (int k = 0; k < K; ++k) v = v + c[k + 1] * (double)S[(int64_t)k * ld + i0 + e];
    out[i0 + e] = (float)v;
  }
}

// ------------------------------------------------------------------------------------------ step 6: llr metrics
// per tile: sum softplus(-llr) over targets, sum softplus(llr) over non-targets (nats; a NaN llr makes its sum NaN), targets,
// NaN llrs, misses (target, llr < theta), false alarms (non-target, llr >= theta): the counts are integers in doubles
constexpr int LM_ACC = 6;
__global__ __launch_bounds__(CAL_THREADS) void llr_partial_kernel(const float* __restrict__ llr, const uint8_t* __restrict__ labels, int64_t P,
                                                                  int vec, double theta, double* __restrict__ partial) {
  double acc[LM_ACC];
#pragma unroll
  for (int a = 0; a < LM_ACC; ++a) acc[a] = 0.0;
  tile_trials<1>(llr, 0, labels, P, vec != 0, [&](const float (&s)[1], bool y) {
    const double z = (double)s[0];
    const bool nan = z != z;
    const double sp = (nan ? z : fmax(y ? -z : z, 0.0)) + log1p(exp(-fabs(z)));
    if (y) acc[0] += sp; else acc[1] += sp;
    acc[2] += y ? 1.0 : 0.0;
    acc[3] += nan ? 1.0 : 0.0;
    acc[4] += y && z < theta ? 1.0 : 0.0;
    acc[5] += !y && z >= theta ? 1.0 : 0.0;
  });
  block_fold_store<LM_ACC>(acc, partial + (int64_t)blockIdx.x * PART_LD);
}

__global__ __launch_bounds__(CAL_THREADS) void llr_finish_kernel(const double* __restrict__ partial, int64_t nblk, int64_t P, double c_miss,
                                                                 double c_fa, double p_target, double* __restrict__ out) {
  __shared__ double tot[PART_LD];
  fold_rows(partial, nblk, LM_ACC, tot);
  if (threadIdx.x != 0) return;
  const double ln2 = 0.6931471805599453;
  const double n_tar = tot[2], n_non = (double)P - n_tar;
  const double cllr_tar = tot[0] / n_tar / ln2, cllr_non = tot[1] / n_non / ln2;
  const double p_miss = tot[4] / n_tar, p_fa = tot[5] / n_non, q_target = 1.0 - p_target;
  const double c_det = __dadd_rn(__dmul_rn(__dmul_rn(c_miss, p_miss), p_target), __dmul_rn(__dmul_rn(c_fa, p_fa), q_target));
  const double c_def = fmin(c_miss * p_target, c_fa * q_target);
  out[0] = 0.5 * (cllr_tar + cllr_non); out[1] = cllr_tar; out[2] = cllr_non; out[3] = c_det / c_def;
  out[4] = p_miss; out[5] = p_fa; out[6] = n_tar; out[7] = tot[3];
}

bool rows_vectorise(const float* S, int64_t ld, int K, const uint8_t* labels) {
  return ((uintptr_t)S & 15) == 0 && (K == 1 || ld % 4 == 0) && (labels == nullptr || ((uintptr_t)labels & 3) == 0);
}

#define CALIB_DISPATCH_K(K_, ...)                          \
  switch (K_) {                                            \
    case 1: { constexpr int KK = 1; __VA_ARGS__; } break;  \
    case 2: { constexpr int KK = 2; __VA_ARGS__; } break;  \
    case 3: { constexpr int KK = 3; __VA_ARGS__; } break;  \
    case 4: { constexpr int KK = 4; __VA_ARGS__; } break;  \
    case 5: { constexpr int KK = 5; __VA_ARGS__; } break;  \
    case 6: { constexpr int KK = 6; __VA_ARGS__; } break;  \
    case 7: { constexpr int KK = 7; __VA_ARGS__; } break;  \
    default: { constexpr int KK = 8; __VA_ARGS__; } break; \
  }

}  // namespace

extern "C" int w2v2_calib_tile(void) { return CAL_TILE; }
extern "C" int w2v2_calib_record_doubles(void) { return R_DOUBLES; }

extern "C" int64_t w2v2_calib_workspace_bytes(int64_t P) {
  return count_ok(P) ? tiles_of(P) * PART_LD * (int64_t)sizeof(double) : -1;
}

extern "C" int w2v2_calib_fit(const float* scores, int64_t ld, int K, const uint8_t* labels, int64_t P, double c_miss, double c_fa,
                              double p_target, double ridge, int max_iter, const double* w_start, double* record, void* workspace,
                              void* stream) {
  W2V2_REQUIRE(count_ok(P), "calib_fit: P = %lld outside [1, 2^31)", (long long)P);
  W2V2_REQUIRE(K >= 1 && K <= MAXK, "calib_fit: K = %d outside [1, %d]", K, MAXK);
  W2V2_REQUIRE(ld >= P, "calib_fit: ld = %lld below P = %lld", (long long)ld, (long long)P);
  W2V2_REQUIRE(scores && labels && record && workspace && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)record & 7) == 0,
               "calib_fit: bad arguments (scores, labels, an 8-byte aligned record and a 16-byte aligned workspace)");
  W2V2_REQUIRE(c_miss >= 1.0 && c_fa >= 1.0 && p_target > 0.0 && p_target < 1.0,
               "calib_fit: c_miss >= 1, c_fa >= 1 and 0 < p_target < 1 (a prior of 0 or 1 has no finite log-odds)");
  W2V2_REQUIRE(ridge >= 0.0 && ridge <= 1.7976931348623157e308, "calib_fit: ridge must be finite and >= 0");
  W2V2_REQUIRE(max_iter >= 1 && max_iter <= 4096, "calib_fit: max_iter = %d outside [1, 4096]", max_iter);
  hipStream_t st = as_stream(stream);
  double* partial = (double*)workspace;
  const int64_t nblk = tiles_of(P);
  const dim3 grid((unsigned)nblk), block(CAL_THREADS);
  const int vec = rows_vectorise(scores, ld, K, labels) ? 1 : 0;
  const double t = p_target * c_miss, pi = t / (t + (1.0 - p_target) * c_fa), tau = log(pi / (1.0 - pi));
  Start start = {};
  if (w_start) {
    start.given = 1;
    for (int a = 0; a <= K; ++a) start.w[a] = w_start[a];
  }
  CALIB_DISPATCH_K(K, hipLaunchKernelGGL(calib_sum_kernel<KK>, grid, block, 0, st, scores, ld, labels, P, vec, partial));
  W2V2_CHECK_LAUNCH("calib_fit(sums)");
  hipLaunchKernelGGL(calib_mean_kernel, dim3(1), block, 0, st, (const double*)partial, nblk, K, P, record);
  W2V2_CHECK_LAUNCH("calib_fit(means)");
  CALIB_DISPATCH_K(K, hipLaunchKernelGGL(calib_dev_kernel<KK>, grid, block, 0, st, scores, ld, labels, P, vec, (const double*)record,
                                         partial));
  W2V2_CHECK_LAUNCH("calib_fit(deviations)");
  hipLaunchKernelGGL(calib_std_kernel, dim3(1), block, 0, st, (const double*)partial, nblk, K, P, start, record);
  W2V2_CHECK_LAUNCH("calib_fit(moments)");
  for (int it = 0; it < max_iter; ++it) {
    CALIB_DISPATCH_K(K, hipLaunchKernelGGL(calib_stats_kernel<KK>, grid, block, 0, st, scores, ld, labels, P, vec, pi, tau,
                                           (const double*)record, partial));
    W2V2_CHECK_LAUNCH("calib_fit(statistics)");
    hipLaunchKernelGGL(calib_solve_kernel, dim3(1), block, 0, st, (const double*)partial, nblk, K, ridge, pi, record);
    W2V2_CHECK_LAUNCH("calib_fit(solve)");
  }
  return 0;
}

extern "C" int w2v2_calib_apply(const float* scores, int64_t ld, int K, int64_t P, const double* a, float* llr_out, void* stream) {
  W2V2_REQUIRE(count_ok(P), "calib_apply: P = %lld outside [1, 2^31)", (long long)P);
  W2V2_REQUIRE(K >= 1 && K <= MAXK, "calib_apply: K = %d outside [1, %d]", K, MAXK);
  W2V2_REQUIRE(ld >= P, "calib_apply: ld = %lld below P = %lld", (long long)ld, (long long)P);
  W2V2_REQUIRE(scores && a && llr_out && ((uintptr_t)a & 7) == 0, "calib_apply: bad arguments (scores, 8-byte aligned a[K + 1], llr_out)");
  const int vec = rows_vectorise(scores, ld, K, nullptr) && ((uintptr_t)llr_out & 15) == 0 ? 1 : 0;
  const dim3 grid((unsigned)cdiv(P, CAL_THREADS * 4)), block(CAL_THREADS);
  CALIB_DISPATCH_K(K, hipLaunchKernelGGL(calib_apply_kernel<KK>, grid, block, 0, as_stream(stream), scores, ld, P, vec, a, llr_out));
  W2V2_CHECK_LAUNCH("calib_apply");
  return 0;
}

extern "C" int w2v2_llr_metrics(const float* llr, const uint8_t* labels, int64_t P, double c_miss, double c_fa, double p_target,
                                double* out, void* workspace, void* stream) {
  W2V2_REQUIRE(count_ok(P), "llr_metrics: P = %lld outside [1, 2^31)", (long long)P);
  W2V2_REQUIRE(llr && labels && out && workspace && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out & 7) == 0,
               "llr_metrics: bad arguments (llr, labels, an 8-byte aligned out[8] and a 16-byte aligned workspace)");
  W2V2_REQUIRE(c_miss >= 1.0 && c_fa >= 1.0 && p_target >= 0.0 && p_target <= 1.0,
               "llr_metrics: c_miss >= 1, c_fa >= 1 and 0 <= p_target <= 1 (calculate_mdc's own conditions)");
  hipStream_t st = as_stream(stream);
  const int64_t nblk = tiles_of(P);
  const double t = p_target * c_miss, pi = t / (t + (1.0 - p_target) * c_fa), theta = -log(pi / (1.0 - pi));
  const int vec = rows_vectorise(llr, 0, 1, labels) ? 1 : 0;
  hipLaunchKernelGGL(llr_partial_kernel, dim3((unsigned)nblk), dim3(CAL_THREADS), 0, st, llr, labels, P, vec, theta, (double*)workspace);
  W2V2_CHECK_LAUNCH("llr_metrics(partials)");
  hipLaunchKernelGGL(llr_finish_kernel, dim3(1), dim3(CAL_THREADS), 0, st, (const double*)workspace, nblk, P, c_miss, c_fa, p_target, out);
  W2V2_CHECK_LAUNCH("llr_metrics(finish)");
  return 0;
}
