// tap_gather.h -- the tap gather of the convolutions that run as "gather, GEMM, adjoint of the gather" and its adjoint, once
// for the three families (tdnn.hip: reflect padding, dilation; wav2spk.hip: zero padding, stride; conv0.hip: stride, no
// padding).  One index map: tap j of output frame t sits at the padded position
//     p(t, j) = t * stride + j * dil - pad
// and a padding policy says what a position outside the L rows of an utterance reads: nothing (PadZero) or the mirrored
// row (PadReflect: ... 2 1 | 0 1 2 ..., torch's "reflect").  Channels-last, one 16-byte StripGeom<T>::Vec per thread,
// grid-stride, no atomics: the adjoint is itself a gather with one writer per vector and a fixed order of additions.
#pragma once
#include "strip_common.h"

// A policy answers, for the gather, which row in [0, L) position p reads (src; a negative value: nothing), and for the
// adjoint, which positions read row s: image(q, s, L, p) sets p to the q-th of IMAGES candidates and says whether it counts.
struct PadZero {
  static constexpr int IMAGES = 1;
  static constexpr bool TOTAL = false;                 // some positions read nothing
  static __device__ __forceinline__ int src(int p, int L) { return p >= 0 && p < L ? p : -1; }
  static __device__ __forceinline__ bool image(int, int s, int, int& p) { p = s; return true; }
};
// (padding < L, the launchers' callers check it: a position is mirrored at most once)
struct PadReflect {
  static constexpr int IMAGES = 3;                     // the position itself, its mirror image left of row 0, right of row L - 1
  static constexpr bool TOTAL = true;                  // every position reads a row
  static __device__ __forceinline__ int src(int p, int L) {
    if (p < 0) p = -p;
    if (p >= L) p = 2 * (L - 1) - p;
    return p;
  }
  static __device__ __forceinline__ bool image(int q, int s, int L, int& p) {
    p = q == 0 ? s : q == 1 ? -s : 2 * (L - 1) - s;
    return q == 0 ? (p >= 0 && p < L) : q == 1 ? (p < 0) : (p >= L);
  }
};

// col[(b,t)][j*Cin + c] = x[b][Pad::src(p(t, j))][c] (+ x2[...]: the taps of x + x2, added once in f32 -- the Res2Net chunk
// input + the previous chunk's output), zeros where the position reads nothing.
// LEN: variable-length batch (evaluation) of a "same" convolution (Tout == Tin), utterance b has lens[b] valid frames.
// The policy sees the utterance's OWN length, so a valid row reads rows < lens[b] only and equals the row of the
// fixed-length form on the [1, lens[b], Cin] slice; rows t >= lens[b] are written as zeros (the products behind them then
// see no padding content).  A workgroup whose 256 vectors all lie in padded rows of one utterance stores its zeros without
// decoding or loading.
template <typename T, typename Pad, bool LEN>
__global__ void tap_gather_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ x2, int64_t ldx2,
                                  T* __restrict__ col, int B, int Tin, int Tout, int Cin, int k, int stride, int dil,
                                  int pad, LensArg<LEN> lens) {
  using Vec = typename StripGeom<T>::Vec;
  constexpr int EPT = StripGeom<T>::EPT;
  const int nch = Cin / EPT;
  const int64_t total = (int64_t)B * Tout * k * nch;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    Vec zero;
#pragma unroll
    for (int e = 0; e < EPT; ++e) zero.v[e] = 0.f;
    if constexpr (LEN) {
      const int64_t per_row = (int64_t)k * nch, i0 = i - threadIdx.x;     // i0: first vector of this workgroup's pass
      const int64_t r0 = i0 / per_row, r1 = (min(i0 + (int64_t)blockDim.x, total) - 1) / per_row;   // first / last row here
      const int b0 = (int)(r0 / Tout);
      if (b0 == (int)(r1 / Tout) && (int)(r0 % Tout) >= lens[b0]) {     // (workgroup-uniform) nothing but padding
        zero.store(col + i * EPT);                                     // col is dense: vector i sits at element i * EPT
        continue;
      }
    }
    const int ch = (int)(i % nch);
    int64_t r = i / nch;
    const int j = (int)(r % k);
    r /= k;
    const int t = (int)(r % Tout), b = (int)(r / Tout);
    T* dst = col + ((int64_t)b * Tout + t) * ((int64_t)k * Cin) + (int64_t)j * Cin + ch * EPT;
    int L = Tin;
    if constexpr (LEN) {
      L = min(lens[b], Tin);
      if (t >= L) {
        zero.store(dst);
        continue;
      }
    }
    int src = Pad::src(t * stride + j * dil - pad, L);
    if constexpr (!Pad::TOTAL)
      if (src < 0) {
        zero.store(dst);
        continue;
      }
    // (the host guarantees padding < lens[b]; the clamp keeps a bad table inside the utterance's rows)
    if constexpr (LEN) src = min(max(src, 0), L - 1);
    Vec v;
    v.load(x + ((int64_t)b * Tin + src) * ldx + ch * EPT);
    if (x2 != nullptr) {
      Vec w;
      w.load(x2 + ((int64_t)b * Tin + src) * ldx2 + ch * EPT);
#pragma unroll
      for (int e = 0; e < EPT; ++e) v.v[e] += w.v[e];
    }
    v.store(dst);
  }
}

// dx[b][s][c] (+)= sum over the (t, j) whose position p(t, j) reads row s of dcol[(b,t)][j*Cin + c].  Taps in ascending
// order, within a tap the policy's images in order, plain f32 adds, one store: bitwise reproducible.
// UNIT: stride == 1 known to the compiler -- the reflect family's launches last 4 to 6 us, and the three inlined
// division sequences of the general form (skipped by a uniform branch, but fetched) cost them 0.4 us
// (profiles/tap_gather_ab.txt).
template <typename T, typename Pad, bool UNIT>
__global__ void tap_adjoint_kernel(const T* __restrict__ dcol, T* __restrict__ dx, int64_t lddx, int B, int Tin, int Tout,
                                   int Cin, int k, int stride, int dil, int pad, int accumulate) {
  using Vec = typename StripGeom<T>::Vec;
  constexpr int EPT = StripGeom<T>::EPT;
  const int nch = Cin / EPT;
  const int64_t total = (int64_t)B * Tin * nch;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % nch);
    const int64_t row = i / nch;
    const int s = (int)(row % Tin), b = (int)(row / Tin);
    float acc[EPT] = {};
    for (int j = 0; j < k; ++j) {
#pragma unroll
      for (int q = 0; q < Pad::IMAGES; ++q) {
        int p;
        if (!Pad::image(q, s, Tin, p)) continue;
        int t = p + pad - j * dil;                     // t * stride, the frame whose tap j sits at p
        if (t < 0) continue;
        if constexpr (!UNIT) {
          if (t % stride != 0) continue;
          t /= stride;
        }
        if (t >= Tout) continue;
        Vec v;
        v.load(dcol + ((int64_t)b * Tout + t) * ((int64_t)k * Cin) + (int64_t)j * Cin + ch * EPT);
#pragma unroll
        for (int e = 0; e < EPT; ++e) acc[e] += v.v[e];
      }
    }
    T* dst = dx + row * lddx + ch * EPT;
    Vec o;
    if (accumulate) {
      o.load(dst);
#pragma unroll
      for (int e = 0; e < EPT; ++e) o.v[e] += acc[e];
    } else {
#pragma unroll
      for (int e = 0; e < EPT; ++e) o.v[e] = acc[e];
    }
    o.store(dst);
  }
}

// ---------------------------------------------------------------- host side
// The checks every caller shares (a 16-byte vector per thread: Cin and the row strides multiples of EPT; the index map's
// frame count); what a family adds (odd k, padding < T, Cin % 8) stays with its entry point.  T: the activation type.
struct TapGeom { int B, Tin, Tout, Cin, k, stride, dil, pad; };
static inline bool tap_geom_ok(const TapGeom& g, int ept) {
  return g.B > 0 && g.Tin > 0 && g.Tout > 0 && g.Cin > 0 && g.Cin % ept == 0 && g.k > 0 && g.stride > 0 && g.dil > 0 &&
         g.pad >= 0;
}
// LEN: the caller's instantiation (W2V2_DISPATCH_LEN), lens non-null exactly then
template <typename T, typename Pad, bool LEN>
static int tap_gather_launch(const char* name, const T* x, int64_t ldx, const T* x2, int64_t ldx2, T* col,
                             const int* lens, const TapGeom& g, void* stream) {
  constexpr int EPT = StripGeom<T>::EPT;
  W2V2_REQUIRE(x && col && tap_geom_ok(g, EPT) && ldx % EPT == 0 && (x2 == nullptr || ldx2 % EPT == 0) &&
                   LEN == (lens != nullptr) && (!LEN || g.Tout == g.Tin),
               "%s: bad arguments (Cin and the row strides multiples of a 16-byte vector; lens: Tout = Tin)", name);
  const int nb = blocks256((int64_t)g.B * g.Tout * g.k * (g.Cin / EPT));
  hipLaunchKernelGGL((tap_gather_kernel<T, Pad, LEN>), dim3(nb), dim3(256), 0, as_stream(stream), x, ldx, x2, ldx2, col,
                     g.B, g.Tin, g.Tout, g.Cin, g.k, g.stride, g.dil, g.pad, lens);
  W2V2_CHECK_LAUNCH(name);
  return 0;
}
template <typename T, typename Pad, bool UNIT>
static int tap_adjoint_launch(const char* name, const T* dcol, T* dx, int64_t lddx, const TapGeom& g, int accumulate,
                              void* stream) {
  constexpr int EPT = StripGeom<T>::EPT;
  W2V2_REQUIRE(dcol && dx && tap_geom_ok(g, EPT) && lddx % EPT == 0 && (!UNIT || g.stride == 1),
               "%s: bad arguments (Cin and the row stride multiples of a 16-byte vector)", name);
  const int nb = blocks256((int64_t)g.B * g.Tin * (g.Cin / EPT));
  hipLaunchKernelGGL((tap_adjoint_kernel<T, Pad, UNIT>), dim3(nb), dim3(256), 0, as_stream(stream), dcol, dx, lddx, g.B, g.Tin,
                     g.Tout, g.Cin, g.k, g.stride, g.dil, g.pad, accumulate);
  W2V2_CHECK_LAUNCH(name);
  return 0;
}
