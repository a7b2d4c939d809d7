// margin_head.hip -- the margin-softmax row kernel with sub-centres, the additive cosine margin and the inter-top-k
// penalty (include/w2v2_hip.h "margin heads": the semantics are defined there, not by a reference file).  It is
// aam_row_kernel (heads.hip) over C classes whose cosine is the maximum of K adjacent sub-centre columns: the same three
// passes, the same 1024-thread stride over the CLASSES and the same fixed-order folds, so that with K = 1, n_top = 0 and
// the angular margin every output has the bits of w2v2_aam_softmax_fwd_bwd.  The products around it (cosine GEMM, d emb,
// aam_dw) are the existing ones over C * K columns.
#include "common.h"

constexpr int MH_THREADS = 1024;          // as AAM_ROW_THREADS: the folds below have its order
constexpr int MH_MAX_K = 8, MH_MAX_TOP = 16;

// m_c = max_k cos[c K + k] and the smallest k that attains it
__device__ __forceinline__ float class_max(const float* __restrict__ cr, int c, int K, int& kstar) {
  const float* p = cr + (int64_t)c * K;
  float m = p[0];
  kstar = 0;
  for (int k = 1; k < K; ++k) {
    const float v = p[k];
    if (v > m) { m = v; kstar = k; }
  }
  return m;
}

// One workgroup per utterance row.  TOPK: the instantiation with the selection rounds and the psi logits; without it the
// body is aam_row_kernel's with class_max in the place of the load.
template <typename T, bool TOPK>
__global__ __launch_bounds__(MH_THREADS) void margin_row_kernel(
    const float* __restrict__ cosv, const int64_t* __restrict__ label, float* __restrict__ softmax,
    float* __restrict__ loss_rows, T* __restrict__ dcos_w, T* __restrict__ dcos_x, const float* __restrict__ inv_x,
    const float* __restrict__ inv_w, float* __restrict__ rowdot, float* __restrict__ colprod, int B, int C, int K,
    int64_t ld, int64_t ldp, float margin, float scale, const float* __restrict__ loss_scale,
    float* __restrict__ correct_rows, int easy_margin, int cos_margin, int n_top, float inter_margin) {
  constexpr int NT = MH_THREADS, NW = NT / 64;
  __shared__ float sh[NW], sh2[NW];
  __shared__ int shi[NW];
  const int b = blockIdx.x;
  const int64_t yl = label[b];
  const bool bad_label = yl < 0 || yl >= C;          // NaN loss for the row, no gradient, no out-of-range read
  const int y = bad_label ? 0 : (int)yl;
  const float* cr = cosv + (int64_t)b * ld;
  float zy, dphi = 1.0f;
  const float sc = scale;
  int ky;
  {
    const float cy = class_max(cr, y, K, ky);
    if (cos_margin) {
      zy = (cy - margin) * scale;                    // AM-softmax / CosFace: phi = cos - m, dphi = 1
    } else {
      const float cos_m = cosf(margin), sin_m = sinf(margin);
      const float th = cosf(3.14159265358979323846f - margin);
      const float mm = sinf(3.14159265358979323846f - margin) * margin;
      const float sine = sqrtf(fminf(fmaxf(1.0f - cy * cy, 0.f), 1.f));
      float phi = cy * cos_m - sine * sin_m;
      if (easy_margin ? (cy > 0.f) : (cy - th > 0.f)) {
        dphi = cos_m + sin_m * cy / fmaxf(sine, 1e-12f);
      } else {
        phi = easy_margin ? cy : cy - mm;
        dphi = 1.0f;
      }
      zy = phi * scale;
    }
  }
  // inter-top-k: n_top rounds of a block arg-max over the classes c != y that come strictly after the previous pick in
  // the order (m descending, c ascending).  After the last round (bv, bi) is the n_top-th pick, and a class is penalised
  // iff it does not come after it: no list is kept.
  float bv = INFINITY;
  int bi = -1;
  const float cos_i = TOPK ? cosf(inter_margin) : 1.0f, sin_i = TOPK ? sinf(inter_margin) : 0.f;
  if constexpr (TOPK) {
    for (int r = 0; r < n_top; ++r) {
      float v = -INFINITY;
      int vi = 0x7fffffff;
      for (int c = threadIdx.x; c < C; c += NT) {
        if (c == y) continue;
        int ks;
        const float m = class_max(cr, c, K, ks);
        if ((m < bv || (m == bv && c > bi)) && m > v) { v = m; vi = c; }     // ascending c: the first maximum stays
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(vi, o, 64);
        if (ov > v || (ov == v && oi < vi)) { v = ov; vi = oi; }
      }
      __syncthreads();
      if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = v; shi[threadIdx.x >> 6] = vi; }
      __syncthreads();
      v = sh[0];
      vi = shi[0];
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const float ov = sh[w];
        const int oi = shi[w];
        if (ov > v || (ov == v && oi < vi)) { v = ov; vi = oi; }
      }
      bv = v;
      bi = vi;
    }
  }
  // the logit of a class c != y from its cosine m; pen: whether it carries the inter-class penalty
  auto off_logit = [&](int c, float m, bool& pen) -> float {
    pen = false;
    if constexpr (TOPK) {
      if (n_top > 0 && (m > bv || (m == bv && c <= bi))) {
        pen = true;
        const float sine = sqrtf(fminf(fmaxf(1.0f - m * m, 0.f), 1.f));
        return (m * cos_i + sine * sin_i) * sc;
      }
    }
    return m * sc;
  };
  float mx = -INFINITY;
  int amax = 0;
  for (int c = threadIdx.x; c < C; c += NT) {
    int ks;
    bool pen;
    const float m = class_max(cr, c, K, ks);
    const float z = c == y ? zy : off_logit(c, m, pen);
    if (z > mx) { mx = z; amax = c; }                  // first maximum of this thread's (ascending) classes
  }
  const float mine = mx;
  mx = block_reduce_n<NW>(mx, sh, true);
  if (correct_rows != nullptr) {
    int cand = (mine == mx) ? amax : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) shi[threadIdx.x >> 6] = cand;
    __syncthreads();
    if (threadIdx.x == 0) {
      int best = shi[0];
#pragma unroll
      for (int w = 1; w < NW; ++w) best = min(best, shi[w]);
      correct_rows[b] = (!bad_label && best == y) ? 1.0f : 0.0f;
    }
  }
  // (sum, sum_off) and the p_y > 1/2 form of the label gradient: see aam_row_kernel
  float sum = 0.f, sum_off = 0.f;
  for (int c = threadIdx.x; c < C; c += NT) {
    int ks;
    bool pen;
    const float m = class_max(cr, c, K, ks);
    const float e = __expf((c == y ? zy : off_logit(c, m, pen)) - mx);
    sum += e;
    if (c != y) sum_off += e;
  }
  block_reduce_sum2<NW>(sum, sum_off, sh, sh2);
  const float inv = 1.0f / sum;
  if (threadIdx.x == 0) loss_rows[b] = bad_label ? __builtin_nanf("") : (mx + __logf(sum)) - zy;
  const float invB = bad_label ? 0.f : (loss_scale ? loss_scale[0] : 1.0f) / (float)B;
  const int64_t Cn = (int64_t)C * K;
  float rd = 0.f;
  for (int c = threadIdx.x; c < C; c += NT) {
    int ks;
    bool pen = false;
    const float cv = class_max(cr, c, K, ks);
    const float p = __expf((c == y ? zy : off_logit(c, cv, pen)) - mx) * inv;
    softmax[(int64_t)b * ldp + c] = p;
    if (dcos_w != nullptr) {
      float g = (p - (c == y ? 1.0f : 0.0f)) * invB * sc;
      if (c == y) {
        if (p > 0.5f) g = -(sum_off * inv) * invB * sc;
        g *= dphi;
      }
      if constexpr (TOPK) {
        if (pen) {
          const float sine = sqrtf(fminf(fmaxf(1.0f - cv * cv, 0.f), 1.f));
          g *= cos_i - sin_i * cv / fmaxf(sine, 1e-12f);
        }
      }
      // g goes to the winning sub-centre's column alone; the class's other columns get exact zeros (one writer each)
      const int64_t col0 = (int64_t)c * K;
      for (int k = 0; k < K; ++k) {
        const int64_t col = col0 + k;
        const bool win = k == ks;
        dcos_w[(int64_t)b * ld + col] = from_f32<T>(win ? (inv_w ? g * inv_w[col] : g) : 0.f);
        if (dcos_x != nullptr) dcos_x[(int64_t)b * ld + col] = from_f32<T>(win ? (inv_x ? g * inv_x[b] : g) : 0.f);
        if (colprod != nullptr) colprod[(int64_t)b * Cn + col] = win ? g * cv : 0.f;
      }
      if (colprod != nullptr) rd = fmaf(g, cv, rd);
    }
  }
  if (rowdot != nullptr && dcos_w != nullptr) {
    rd = block_reduce_n<NW>(rd, sh, false);
    if (threadIdx.x == 0) rowdot[b] = rd;
  }
}

extern "C" int w2v2_margin_softmax_fwd_bwd(const float* cos, const int64_t* label, float* softmax, float* loss_rows,
                                           void* dcos_w, void* dcos_x, const float* inv_x, const float* inv_w,
                                           float* rowdot, float* colprod, int B, int C, int K, int64_t ld, int64_t ldp,
                                           float margin, float scale, int easy_margin, int margin_type, int n_top,
                                           float inter_margin, const float* loss_scale, float* correct_rows, int dtype,
                                           void* stream) {
  W2V2_REQUIRE(cos && label && softmax && loss_rows && B > 0 && C > 0, "margin_softmax: bad arguments");
  W2V2_REQUIRE(K >= 1 && K <= MH_MAX_K, "margin_softmax: %d sub-centres outside [1, %d]", K, MH_MAX_K);
  W2V2_REQUIRE((int64_t)C * K <= 0x7fffffff && ld >= (int64_t)C * K && ldp >= C,
               "margin_softmax: row strides %lld / %lld under %d x %d columns / %d classes", (long long)ld, (long long)ldp,
               C, K, C);
  W2V2_REQUIRE(margin_type == 0 || margin_type == 1, "margin_softmax: margin type %d is neither ARC (0) nor COS (1)",
               margin_type);
  W2V2_REQUIRE(margin >= 0.f || margin_type == 1, "margin_softmax: a negative angular margin (the plain head is "
               "w2v2_aam_softmax_fwd_bwd's)");
  W2V2_REQUIRE(n_top >= 0 && n_top <= MH_MAX_TOP && n_top <= C - 1,
               "margin_softmax: inter-top-k %d outside [0, min(%d, %d)]", n_top, C - 1, MH_MAX_TOP);
  W2V2_REQUIRE(inter_margin >= 0.f, "margin_softmax: negative inter-class margin %g", (double)inter_margin);
  hipStream_t st = as_stream(stream);
  W2V2_DISPATCH_ACT(dtype, "margin_softmax", {
    if (n_top > 0)
      hipLaunchKernelGGL((margin_row_kernel<AT, true>), dim3(B), dim3(MH_THREADS), 0, st, cos, label, softmax, loss_rows,
                         (AT*)dcos_w, (AT*)dcos_x, inv_x, inv_w, rowdot, colprod, B, C, K, ld, ldp, margin, scale,
                         loss_scale, correct_rows, easy_margin, margin_type, n_top, inter_margin);
    else
      hipLaunchKernelGGL((margin_row_kernel<AT, false>), dim3(B), dim3(MH_THREADS), 0, st, cos, label, softmax, loss_rows,
                         (AT*)dcos_w, (AT*)dcos_x, inv_x, inv_w, rowdot, colprod, B, C, K, ld, ldp, margin, scale,
                         loss_scale, correct_rows, easy_margin, margin_type, n_top, inter_margin);
  });
  W2V2_CHECK_LAUNCH("margin_softmax");
  return 0;
}
