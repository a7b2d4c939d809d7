// ctc_long.hip -- the CTC loss for transcripts (ref: src/lightning_modules/speech/speech_recognition_module.py:100-116 with
// src/optim/loss/ctc_loss.py:36-58): up to 1023 labels per utterance, where ctc.hip stops at the 31 that fit one
// wavefront.  Same contract, same three launches, same arithmetic (ctc_common.h); what differs is who owns a state:
//   ctc_long_row_kernel      row statistics of a frame and its L + 1 emission slots, the slots in a loop over the workgroup
//   ctc_long_lattice_kernel  one workgroup of 64 ... 1024 threads per utterance.  Thread j owns the PAIR (blank state 2j,
//                            label state 2j + 1): the s - 1 neighbour of a label is in the same thread, and one (m, e)
//                            pair per thread and frame crosses threads forward (the previous thread's label state, s - 1
//                            of the blank and s - 2 of the label), two backward (the next thread's blank and label).  They
//                            go through a double-buffered LDS slot per thread: one barrier per frame.  The backward pass
//                            turns alpha into the state posterior IN PLACE, so the workspace holds 8 bytes per state and
//                            frame, not the 16 of alpha and beta.
//   ctc_long_grad_kernel     dense gradient row.  Repeated labels are merged along a chain (next occurrence of the same
//                            class) that the lattice kernel builds once per utterance: the first occurrence walks it in
//                            ascending order and is the one writer of its class column, O(L) per frame in all.  The
//                            class -> posterior map lives in LDS a tile of 4096 columns at a time, so a column costs one
//                            LDS read whatever L is.
// and the greedy decoder of the speech step (ref: speech_recognition_module.py:233-248): ctc_greedy_kernel.
#include "ctc_common.h"

constexpr int CTCL_MAX_L = 1023;          // L + 1 <= 1024 threads
constexpr int CTCL_STAGE = 3072;          // emission slots staged in LDS per chunk of frames (2 x 12 KiB)
constexpr int CTCL_MAX_THREADS = 1024;
constexpr int CTCL_TILE = 4096;           // class columns whose merged posteriors are in LDS at a time (16 KiB)

// the caller's workspace, cut up (4-byte elements; every part starts 16-byte aligned)
struct CtcLongWs {
  float4* info;      // [B]     {P mantissa, P exponent (int bits), status: 0 ok / 1 infeasible / 2 bad row, -}
  float4* rowstat;   // [rows]  {row max, 1 / sum exp, off-blank softmax mass, -}
  int* chain;        // [B][2][W4]  next label of the same class (-1: none); class of a FIRST occurrence (-1: a later one)
  float* pm;         // [rows][W + 1]   emission probability of slot k (0 = blank, k = target k - 1): mantissa in [1, 2)
  int* pe;           //                 ... and exponent
  float4* alpha;     // [rows][W + 1]   thread j's pair {blank m, e (int bits), label m, e}; after the backward pass the
                     //                 two mantissas are the state posteriors
};
static __host__ __device__ inline int ctcl_w4(int W) { return (W + 3) & ~3; }
static __host__ __device__ inline int64_t ctcl_slots(int64_t rows, int W) { return (2 * rows * (W + 1) + 3) & ~(int64_t)3; }
static __host__ __device__ inline int64_t ctcl_ws_floats(int B, int64_t rows, int W) {
  return 4 * (int64_t)B + 4 * rows + 2 * (int64_t)B * ctcl_w4(W) + ctcl_slots(rows, W) + 4 * rows * (W + 1);
}
static inline CtcLongWs ctcl_carve(float* ws, int B, int64_t rows, int W) {
  CtcLongWs w;
  float* p = ws;
  w.info = reinterpret_cast<float4*>(p); p += 4 * (int64_t)B;
  w.rowstat = reinterpret_cast<float4*>(p); p += 4 * rows;
  w.chain = reinterpret_cast<int*>(p); p += 2 * (int64_t)B * ctcl_w4(W);
  w.pm = p;
  w.pe = reinterpret_cast<int*>(p + rows * (W + 1)); p += ctcl_slots(rows, W);
  w.alpha = reinterpret_cast<float4*>(p);
  return w;
}
static inline int ctcl_threads(int W) {          // the smallest workgroup with a thread for every pair: L + 1 <= threads
  int nt = 64;
  while (nt < W + 1) nt <<= 1;
  return nt;
}

__global__ __launch_bounds__(CTC_ROW_THREADS) void ctc_long_row_kernel(const float* __restrict__ logits, int64_t ldc,
                                                                       const int64_t* __restrict__ targets, int64_t tstride,
                                                                       int W, int toff, const int* __restrict__ in_len,
                                                                       const int* __restrict__ tgt_len, int blank,
                                                                       CtcLongWs ws, int T, int C) {
  ctc_row_pass<true>(logits, ldc, targets, tstride, W, toff, in_len, tgt_len, blank, ws.rowstat, ws.pm, ws.pe, T, C);
}

// the value 0 in both (m, e) pairs of a thread.  (A function, not a named constant: a float4 object that is selected
// against an LDS or global load ends up in scratch.)
__device__ __forceinline__ float4 ctcl_zero4() {
  return make_float4(0.f, __int_as_float(CTC_ZERO_E), 0.f, __int_as_float(CTC_ZERO_E));
}

__global__ __launch_bounds__(CTCL_MAX_THREADS) void ctc_long_lattice_kernel(const int64_t* __restrict__ targets,
                                                                            int64_t tstride, int W, int toff,
                                                                            const int* __restrict__ in_len,
                                                                            const int* __restrict__ tgt_len, int blank,
                                                                            CtcLongWs ws, float* __restrict__ loss_rows, int T,
                                                                            int C) {
  __shared__ float pm_s[CTCL_STAGE];
  __shared__ int pe_s[CTCL_STAGE];
  __shared__ float4 x_s[2][CTCL_MAX_THREADS];     // what crosses threads, double-buffered: one barrier per frame
  __shared__ float fin_s[4];
  const int b = blockIdx.x, j = threadIdx.x, NT = blockDim.x;       // (the host launches NT >= W + 1)
  const int Tb = in_len[b], L = tgt_len[b];
  const bool badlen = ctc_bad_lengths(Tb, L, T, W);
  const int64_t* trow = targets + (int64_t)b * tstride;
  bool badt = false;
  int cls = -1;
  if (!badlen && j < L) cls = ctc_state_class(trow, 2 * j + 1, 2 * L + 1, toff, blank, C, badt);
  if (__syncthreads_or(badlen || badt)) {      // NaN loss row, zero gradient (the bad_label convention of aam_row_kernel)
    if (j == 0) {
      loss_rows[b] = __builtin_nanf("");
      ws.info[b] = make_float4(0.f, 0.f, 2.f, 0.f);
    }
    return;
  }
  // the classes of the neighbouring labels, and the chain of repeated labels for the gradient pass (once per utterance;
  // the staging buffer is free until the first chunk)
  int* cls_s = pe_s;
  int* first_s = pe_s + CTCL_MAX_THREADS;
  cls_s[j] = cls;                              // (-1 from j = L on: matches no class)
  first_s[j] = 1;
  __syncthreads();
  const int clsp = j >= 1 ? cls_s[j - 1] : -1, clsn = j + 1 < NT ? cls_s[j + 1] : -1;
  int nxt = -1;
  if (j < L) {
    for (int i = j + 1; i < L; ++i)
      if (cls_s[i] == cls) { nxt = i; break; }
    if (nxt >= 0) first_s[nxt] = 0;            // (one writer: only the occurrence before it points at a label)
  }
  __syncthreads();
  const int W4 = ctcl_w4(W);
  if (j < L) {
    ws.chain[(int64_t)b * 2 * W4 + j] = nxt;
    ws.chain[(int64_t)b * 2 * W4 + W4 + j] = first_s[j] ? cls : -1;
  }
  const bool live_b = j <= L, live_l = j < L;
  const bool skip_to = j >= 1 && live_l && cls != clsp;          // s - 2 -> s (different labels only)
  const bool skip_from = j + 1 < L && clsn != cls;               // s -> s + 2
  const int W1 = W + 1;
  const int slot = live_l ? j + 1 : 0;
  const int64_t row0 = (int64_t)b * T;
  const int nfmax = CTCL_STAGE / W1;
  // alpha: the virtual column before frame 0 holds 1 in state 0, so frame 0 needs no case of its own
  CtcME ab = j == 0 ? CtcME{0.5f, 1} : ctc_zero(), al = ctc_zero();
  int g = 0;
  x_s[0][j] = ctcl_zero4();
  for (int t0 = 0; t0 < Tb; t0 += nfmax) {
    const int nf = min(nfmax, Tb - t0);
    __syncthreads();
    for (int i = j; i < nf * W1; i += NT) {
      pm_s[i] = ws.pm[(row0 + t0) * W1 + i];
      pe_s[i] = ws.pe[(row0 + t0) * W1 + i];
    }
    for (int f = 0; f < nf; ++f) {
      __syncthreads();
      const float4 q = x_s[g & 1][max(j - 1, 0)];
      const CtcME pl = j >= 1 ? CtcME{q.z, __float_as_int(q.w)} : ctc_zero();      // the previous thread's label state at t - 1
      const CtcME vb = ctc_sum3(ab, pl, ctc_zero());
      const CtcME vl = ctc_sum3(al, ab, skip_to ? pl : ctc_zero());
      ab = live_b ? ctc_norm(vb.m * pm_s[f * W1], vb.e + pe_s[f * W1]) : ctc_zero();
      al = live_l ? ctc_norm(vl.m * pm_s[f * W1 + slot], vl.e + pe_s[f * W1 + slot]) : ctc_zero();
      ++g;
      const float4 mine = make_float4(ab.m, __int_as_float(ab.e), al.m, __int_as_float(al.e));
      x_s[g & 1][j] = mine;
      if (j <= W) ws.alpha[(row0 + t0 + f) * W1 + j] = mine;
    }
  }
  // P = alpha_{Tb-1}(S - 1) + alpha_{Tb-1}(S - 2): the blank of thread L and the label of thread L - 1
  __syncthreads();
  if (j == L) { fin_s[0] = ab.m; fin_s[1] = __int_as_float(ab.e); }
  if (j == max(L - 1, 0)) {
    const CtcME v = L >= 1 ? al : ctc_zero();
    fin_s[2] = v.m; fin_s[3] = __int_as_float(v.e);
  }
  __syncthreads();
  const CtcME pv = ctc_sum3(CtcME{fin_s[0], __float_as_int(fin_s[1])}, CtcME{fin_s[2], __float_as_int(fin_s[3])}, ctc_zero());
  const CtcME P = ctc_norm(pv.m, pv.e);
  if (j == 0) {
    // zero_infinity: an infeasible utterance (P = 0) contributes 0 to the loss and to the gradient
    const bool feasible = P.m > 0.f;
    loss_rows[b] = feasible ? -fmaf((float)P.e, 0.69314718055994531f, logf(P.m)) / (float)max(L, 1) : 0.f;
    ws.info[b] = make_float4(P.m, __int_as_float(P.e), feasible ? 0.f : 1.f, 0.f);
  }
  if (!(P.m > 0.f) || Tb == 0) return;
  // beta~_t(s): everything after frame t, WITHOUT the emission at t; beta~_{Tb-1} = 1 in the two final states.  With
  // alpha_t(s) of the forward pass it gives the posterior of the state, which takes alpha's place in the workspace.
  CtcME bb = j == L ? CtcME{0.5f, 1} : ctc_zero(), bl = j == L - 1 ? CtcME{0.5f, 1} : ctc_zero();
  const int nchunk = (Tb + nfmax - 1) / nfmax;
  float4 a = ctcl_zero4();
  if (j <= W) a = ws.alpha[(row0 + Tb - 1) * W1 + j];
  for (int ch = nchunk - 1; ch >= 0; --ch) {
    const int t0 = ch * nfmax, nf = min(nfmax, Tb - t0);
    __syncthreads();
    for (int i = j; i < nf * W1; i += NT) {
      pm_s[i] = ws.pm[(row0 + t0) * W1 + i];
      pe_s[i] = ws.pe[(row0 + t0) * W1 + i];
    }
    __syncthreads();
    for (int f = nf - 1; f >= 0; --f) {
      const int t = t0 + f;
      float4 an = ctcl_zero4();
      if (j <= W && t > 0) an = ws.alpha[(row0 + t - 1) * W1 + j];                         // (a frame ahead of its use)
      if (j <= W) {
        const float gam_b = ctc_posterior(a.x, __float_as_int(a.y), bb.m, bb.e, P.m, P.e);
        const float gam_l = ctc_posterior(a.z, __float_as_int(a.w), bl.m, bl.e, P.m, P.e);
        ws.alpha[(row0 + t) * W1 + j] = make_float4(gam_b, a.y, gam_l, a.w);
      }
      const CtcME fb = live_b ? CtcME{bb.m * pm_s[f * W1], bb.m > 0.f ? bb.e + pe_s[f * W1] : CTC_ZERO_E} : ctc_zero();
      const CtcME fl = live_l ? CtcME{bl.m * pm_s[f * W1 + slot], bl.m > 0.f ? bl.e + pe_s[f * W1 + slot] : CTC_ZERO_E}
                              : ctc_zero();
      ++g;
      x_s[g & 1][j] = make_float4(fb.m, __int_as_float(fb.e), fl.m, __int_as_float(fl.e));
      __syncthreads();
      const float4 q = x_s[g & 1][min(j + 1, NT - 1)];
      const bool has = j + 1 < NT;
      const CtcME nb = has ? CtcME{q.x, __float_as_int(q.y)} : ctc_zero(), nl = has ? CtcME{q.z, __float_as_int(q.w)} : ctc_zero();
      const CtcME vb = ctc_sum3(fb, fl, ctc_zero());
      const CtcME vl = ctc_sum3(fl, nb, skip_from ? nl : ctc_zero());
      bb = live_b ? ctc_norm(vb.m, vb.e) : ctc_zero();
      bl = live_l ? ctc_norm(vl.m, vl.e) : ctc_zero();
      a = an;
    }
  }
}

template <typename TG>
__global__ __launch_bounds__(CTC_ROW_THREADS) void ctc_long_grad_kernel(const float* __restrict__ logits, int64_t ldc, int W,
                                                                        const int* __restrict__ in_len,
                                                                        const int* __restrict__ tgt_len, int blank,
                                                                        CtcLongWs ws, TG* __restrict__ dl,
                                                                        const float* __restrict__ loss_scale, int B, int T,
                                                                        int C) {
  constexpr int NT = CTC_ROW_THREADS, NW = NT / 64, NL = CTCL_MAX_THREADS / NT;
  __shared__ float map_s[CTCL_TILE], gl_s[CTCL_MAX_THREADS], sha[NW], shb[NW];
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
  const int L = tgt_len[b], S = 2 * L + 1;
  // the posteriors of the frame: the two sums off and on the labels, the label ones kept for the chains
  const float2* grow = reinterpret_cast<const float2*>(ws.alpha + r * (W + 1));
  float gb = 0.f, gl = 0.f;
  for (int s = tid; s < S; s += NT) {          // (NT is even: a thread sees states of one parity)
    const float g = grow[s].x;
    if (s & 1) { gl += g; gl_s[s >> 1] = g; }
    else gb += g;
  }
  block_reduce_sum2<NW>(gb, gl, sha, shb);     // (its barriers publish gl_s)
  // repeated labels share a class: the first occurrence carries the sum of their posteriors (ascending order), the later
  // ones match no column -- one writer per gradient element
  const int W4 = ctcl_w4(W);
  const int* nxt = ws.chain + (int64_t)b * 2 * W4;
  const int* fcls = nxt + W4;
  float occ[NL];
  int oc[NL];
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const int l = tid + k * NT;
    oc[k] = -1;
    occ[k] = 0.f;
    if (l < L) {
      oc[k] = fcls[l];
      if (oc[k] >= 0) {
        float s = 0.f;
        for (int i = l; i >= 0; i = nxt[i]) s += gl_s[i];
        occ[k] = s;
      }
    }
  }
  const float4 rs = ws.rowstat[r];
  const float mx = rs.x, inv = rs.y, offm = rs.z;
  const float k = (loss_scale ? loss_scale[0] : 1.0f) / ((float)B * (float)max(L, 1));
  const float* zr = logits + r * ldc;
  const float4* z4 = reinterpret_cast<const float4*>(zr);
  for (int c0 = 0; c0 < C; c0 += CTCL_TILE) {
    const int nc = min(CTCL_TILE, C - c0);
    if (c0 > 0) __syncthreads();
    for (int i = tid; i < nc; i += NT) map_s[i] = 0.f;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NL; ++q)
      if (oc[q] >= c0 && oc[q] < c0 + nc) map_s[oc[q] - c0] = occ[q];
    __syncthreads();
    auto grad = [&](int c, float z) -> float {
      const float p = ctc_exp(z - mx) * inv;
      // softmax[blank] and gamma(blank) both 1 - small under the reference's blank bias: p - gamma from the two small
      // sums, sum_label gamma - sum_{c != blank} softmax_c
      const float g = c == blank ? (p > 0.5f ? gl - offm : p - gb) : p - map_s[c - c0];
      return g * k;
    };
    if (vec) {
      for (int v = (c0 >> 2) + tid; v < ((c0 + nc + 3) >> 2); v += NT) {
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
      for (int c = c0 + tid; c < c0 + nc; c += NT) dr[c] = from_f32<TG>(grad(c, zr[c]));
    }
  }
}

// Greedy decoding: one workgroup per utterance, a thread per frame in chunks of 256 frames.  argmax over c < C (the lowest
// index wins a tie), a frame is kept when its index differs from the previous frame's and is not the blank (collapse,
// THEN drop: `a a _ a` gives `a a`), and the kept ones are written in frame order at the positions a ballot and a prefix
// over the four waves give them.  No atomics.
__global__ __launch_bounds__(CTC_ROW_THREADS) void ctc_greedy_kernel(const float* __restrict__ logits, int64_t ldc,
                                                                     const int* __restrict__ in_len, int blank, int T, int C,
                                                                     int* __restrict__ tokens, int* __restrict__ counts) {
  constexpr int NT = CTC_ROW_THREADS, NW = NT / 64;
  __shared__ int arg_s[NT], tot_s[NW];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tb = in_len[b];
  if (Tb < 0 || Tb > T) {                      // (block-uniform) a bad length: count -1, nothing read
    if (tid == 0) counts[b] = -1;
    return;
  }
  const bool vec = (ldc & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
  int count = 0, carry = -1;
  for (int t0 = 0; t0 < Tb; t0 += NT) {
    const int t = t0 + tid;
    int a = -1;
    if (t < Tb) {
      const float* zr = logits + ((int64_t)b * T + t) * ldc;
      float best = zr[0];
      a = 0;
      if (vec) {
        const float4* z4 = reinterpret_cast<const float4*>(zr);
        for (int v = 0; v < ((C + 3) >> 2); ++v) {
          const float4 q = z4[v];
          const float z[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (4 * v + i < C && z[i] > best) { best = z[i]; a = 4 * v + i; }
        }
      } else {
        for (int c = 1; c < C; ++c)
          if (zr[c] > best) { best = zr[c]; a = c; }
      }
    }
    arg_s[tid] = a;
    __syncthreads();
    const int prev = tid > 0 ? arg_s[tid - 1] : carry;
    const bool keep = t < Tb && a != prev && a != blank;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) tot_s[wave] = __popcll(bal);
    __syncthreads();
    int off = count, total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      if (w < wave) off += tot_s[w];
      total += tot_s[w];
    }
    if (keep) tokens[(int64_t)b * T + off + __popcll(bal & ((1ull << lane) - 1ull))] = a;
    count += total;
    carry = arg_s[NT - 1];
    __syncthreads();                           // before the next chunk rewrites arg_s and tot_s
  }
  if (tid == 0) counts[b] = count;
}

extern "C" int64_t w2v2_ctc_long_workspace_floats(int B, int T, int target_width) {
  if (B <= 0 || T <= 0 || target_width < 0 || target_width > CTCL_MAX_L) return -1;
  return ctcl_ws_floats(B, (int64_t)B * T, target_width);
}

extern "C" int w2v2_ctc_long_stage_frames(int target_width) {
  if (target_width < 0 || target_width > CTCL_MAX_L) return -1;
  return CTCL_STAGE / (target_width + 1);
}

extern "C" int w2v2_ctc_long_fwd_bwd(const float* logits, int64_t ldc, const int64_t* targets, int64_t target_stride,
                                     int target_width, int target_offset, const int* input_lengths,
                                     const int* target_lengths, int blank, float* loss_rows, void* dlogits,
                                     const float* loss_scale, float* workspace, int64_t workspace_floats, int B, int T, int C,
                                     int dtype, void* stream) {
  W2V2_REQUIRE(logits && input_lengths && target_lengths && loss_rows && workspace && B > 0 && T > 0 && C > 0 && ldc >= C,
               "ctc_long: bad arguments");
  W2V2_REQUIRE(target_width >= 0 && target_width <= CTCL_MAX_L,
               "ctc_long: targets of width %d; the lattice of one utterance is one workgroup (at most %d labels)",
               target_width, CTCL_MAX_L);
  W2V2_REQUIRE(targets != nullptr || target_width == 0, "ctc_long: no targets");
  W2V2_REQUIRE(target_stride >= 0 && blank >= 0 && blank < C,
               "ctc_long: blank %d outside [0, %d) or a negative target stride", blank, C);
  const int64_t rows = (int64_t)B * T;
  W2V2_REQUIRE(rows < (int64_t)1 << 31, "ctc_long: %lld rows", (long long)rows);
  W2V2_REQUIRE(workspace_floats >= ctcl_ws_floats(B, rows, target_width) && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
               "ctc_long: the workspace needs %lld floats (w2v2_ctc_long_workspace_floats), 16-byte aligned",
               (long long)ctcl_ws_floats(B, rows, target_width));
  const CtcLongWs ws = ctcl_carve(workspace, B, rows, target_width);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ctc_long_row_kernel, dim3((unsigned)rows), dim3(CTC_ROW_THREADS), 0, st, logits, ldc, targets,
                     target_stride, target_width, target_offset, input_lengths, target_lengths, blank, ws, T, C);
  hipLaunchKernelGGL(ctc_long_lattice_kernel, dim3(B), dim3(ctcl_threads(target_width)), 0, st, targets, target_stride,
                     target_width, target_offset, input_lengths, target_lengths, blank, ws, loss_rows, T, C);
  if (dlogits != nullptr) {
    W2V2_DISPATCH_ACT(dtype, "ctc_long",
      hipLaunchKernelGGL(ctc_long_grad_kernel<AT>, dim3((unsigned)rows), dim3(CTC_ROW_THREADS), 0, st, logits, ldc,
                         target_width, input_lengths, target_lengths, blank, ws, (AT*)dlogits, loss_scale, B, T, C););
  }
  W2V2_CHECK_LAUNCH("ctc_long");
  return 0;
}

extern "C" int w2v2_ctc_greedy_decode(const float* logits, int64_t ldc, const int* input_lengths, int blank, int B, int T,
                                      int C, int* tokens_out, int* counts_out, void* stream) {
  W2V2_REQUIRE(logits && input_lengths && tokens_out && counts_out && B > 0 && T > 0 && C > 0 && ldc >= C,
               "ctc_greedy_decode: bad arguments");
  W2V2_REQUIRE((int64_t)B * T < (int64_t)1 << 31, "ctc_greedy_decode: %lld rows", (long long)B * T);
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(CTC_ROW_THREADS), 0, as_stream(stream), logits, ldc, input_lengths,
                     blank, T, C, tokens_out, counts_out);
  W2V2_CHECK_LAUNCH("ctc_greedy_decode");
  return 0;
}
