// Reverb augmentation on the device (f32, gfx950, wave64): sox's freeverb bank -- per output channel 8 damped feedback
// combs summed, then 4 all-passes in series -- for `augment_add_reverb`.  include/w2v2_hip.h, "waveform augmentation",
// is the definition; the conventions of augment.hip hold (rows by list, zero by index behind len, row * ld in 64 bits,
// no atomics, one writer per element, nothing allocated, everything on the caller's stream).
//
// What is sequential and what is not.  A comb of delay D reads what it wrote D samples ago, so D consecutive samples
// have their delay-line outputs o[n] in hand at once; the only lag-1 dependency is the one-pole low-pass in the feedback,
//   store[n] = o[n] + (store[n - 1] - o[n]) damp = damp store[n - 1] + (o[n] - o[n] damp),
// a first-order linear recurrence with a constant ratio: a scan.  An all-pass of delay D is a pure lag-D recurrence.
//
// One workgroup of 16 waves owns one listed row from start to end.  The 24 delay lines stay in LDS for the whole row,
// the 16 comb `store` values in registers; the row is walked in chunks of RV_CHUNK samples:
//   combs   wave i = comb (array i / 8, comb i % 8) walks chunk k (staged in xs, zero by index behind len) in SEGMENTS that
//           end where its delay line wraps (n a multiple of D) or the chunk ends; a segment is taken 64 samples at a time:
//           read o from the line, scan the low-pass across the wave with the carried store folded in, write
//           x + store feedback back to the line
//   allpass the cascade 3 .. 0 is a pipeline over chunks: wave 4 w + s (s < 4) runs array w's all-pass 3 - s over chunk
//           k - 1 - s in place, in segments of its delay, in the same interval as the combs; five chunk slots are in flight
//   -- barrier --
//   sum     comb outputs of chunk k added in the defined order 7 .. 0, into the chunk's slot
//   out     y = 0.5 ((dry x + wet_0) + (dry x + wet_1)) for chunk k - 4, which has left the last all-pass
//   stage   chunk k + 1 of the source -> xs
//   -- barrier --
// so a chunk costs two barriers, and the 8 all-passes run beside each other and behind the combs' waves, not after them.
// The scan has two levels.  Within a row of 16 lanes it is Kogge-Stone on the right-hand sides b[n] = o[n] - o[n] damp
// alone: b += damp^(2^k) (b of the lane 2^k below, zeros shifted in at the row's start), k = 0 .. 3, the powers by repeated
// squaring in f32.  The state in front of row q + 1 is S[q + 1] = damp^16 S[q] + b[16 q + 15] with S[0] the carried store,
// and store = b + damp^(lane % 16 + 1) S[row].  Segment and chunk boundaries are functions of the delay and of RV_CHUNK,
// never of B, N, R or the grid, and a sample's value depends on no later sample: a row is bit-identical to the same call
// on the row alone, and cropping at N_out < len returns the same leading samples.
#include "common.h"

namespace {

constexpr int RV_CHUNK = 512, RV_THREADS = 1024, RV_MAXD = W2V2_AUG_REVERB_MAX_DELAY;
constexpr int RV_COMBS = 16, RV_APS = 8;                    // 2 arrays x 8 combs, 2 arrays x 4 all-passes
constexpr int RV_AP_STAGES = 4, RV_AP_SLOTS = RV_AP_STAGES + 1;      // chunks k - 4 .. k are in flight at once
constexpr int RV_P_COMB = 0, RV_P_AP = 16, RV_P_FEEDBACK = 24, RV_P_DAMP = 25, RV_P_WET = 26, RV_P_DRY = 27;
static_assert(W2V2_AUG_REVERB_PARAMS == 28, "16 comb delays, 8 all-pass delays, feedback, damp, wet gain, dry gain");
static_assert(RV_THREADS == 64 * RV_COMBS && RV_THREADS == 2 * RV_CHUNK, "a wave per comb, a thread per (array, sample) of a chunk");
static_assert(((RV_COMBS + RV_APS) * RV_MAXD + (RV_COMBS + 2 * RV_AP_SLOTS + 1) * RV_CHUNK) * 4 <= 160 * 1024, "the LDS of one CU");

__device__ __forceinline__ float rv_qnan() { return __uint_as_float(0x7fc00000u); }

// v of the lane SH below in the same row of 16 lanes (DPP row_shr), 0.0f in the lanes that have none
template <int SH>
__device__ __forceinline__ float rv_row_shr(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x110 + SH, 0xf, 0xf, true));
}
__device__ __forceinline__ float rv_lane(float v, int l) {    // lane l's v in every lane (l wave-uniform)
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// LDS traffic between the lanes of ONE wave: what a segment wrote, the next one reads from other lanes
__device__ __forceinline__ void rv_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(RV_THREADS) void aug_reverb_kernel(const float* __restrict__ src, int64_t ld_src, int N_in,
                                                                const int* __restrict__ lens, const int* __restrict__ src_rows,
                                                                float* __restrict__ dst, int64_t ld_dst, int N_out,
                                                                const int* __restrict__ dst_rows, const int* __restrict__ params) {
  __shared__ float line[RV_COMBS][RV_MAXD];                  // comb delay lines, position n mod D
  __shared__ float apl[RV_APS][RV_MAXD];                     // all-pass delay lines
  __shared__ float co[RV_COMBS][RV_CHUNK];                   // comb outputs of the chunk
  __shared__ float ap[2][RV_AP_SLOTS][RV_CHUNK];             // per chunk in flight: the comb sums, then the cascade in place
  __shared__ float xs[RV_CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, r = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform, and known to be: delays and trip counts are scalars
  const int srow = src_rows[r], drow = dst_rows[r];
  const int* __restrict__ pr = params + (int64_t)r * W2V2_AUG_REVERB_PARAMS;
  float* __restrict__ y = dst + (int64_t)drow * ld_dst;
  const float* __restrict__ x = src + (int64_t)srow * ld_src;
  int len = lens ? lens[srow] : N_in;
  len = min(max(len, 0), N_in);
  const int live = min(len, N_out);                          // outputs [0, live) are filtered, [live, N_out) zeros

  bool bad = false;
  for (int i = 0; i < RV_COMBS + RV_APS; ++i) bad |= pr[i] < 1 || pr[i] > RV_MAXD;      // (workgroup-uniform)
  if (bad || live == 0) {
    const float fill = bad ? rv_qnan() : 0.0f;
    for (int n = tid; n < N_out; n += RV_THREADS) y[n] = fill;
    return;
  }
  const float feedback = __int_as_float(pr[RV_P_FEEDBACK]), damp = __int_as_float(pr[RV_P_DAMP]);
  const float wet_gain = __int_as_float(pr[RV_P_WET]), dry_gain = __int_as_float(pr[RV_P_DRY]);
  const int D = pr[RV_P_COMB + wave];                        // this wave's comb
  // damp^(2^k) by squaring, and damp^(lane % 16 + 1) as the product of the squares its bits name, lowest first
  const float d1 = damp, d2 = d1 * d1, d4 = d2 * d2, d8 = d4 * d4, d16 = d8 * d8;
  const int row = lane >> 4, e = (lane & 15) + 1;
  float dlane = 1.0f;
  if (e & 1) dlane *= d1;
  if (e & 2) dlane *= d2;
  if (e & 4) dlane *= d4;
  if (e & 8) dlane *= d8;
  if (e & 16) dlane *= d16;
  for (int i = tid; i < RV_COMBS * RV_MAXD; i += RV_THREADS) (&line[0][0])[i] = 0.0f;
  for (int i = tid; i < RV_APS * RV_MAXD; i += RV_THREADS) (&apl[0][0])[i] = 0.0f;
  float store = 0.0f;                                        // the comb's low-pass state, the same in every lane

  // waves 0 .. 7 also own one all-pass: array apw, stage aps (stage 0 is all-pass 3, the first in the cascade)
  const int apw = (wave >> 2) & 1, aps = wave & 3;
  const int Da = pr[RV_P_AP + apw * 4 + (3 - aps)];
  float* __restrict__ aline = apl[apw * 4 + (3 - aps)];
  const int nchunks = (live + RV_CHUNK - 1) / RV_CHUNK;
  if (tid < RV_CHUNK) xs[tid] = tid < live ? x[tid] : 0.0f;
  __syncthreads();

  for (int k = 0; k < nchunks + RV_AP_STAGES; ++k) {
    // ---- combs on chunk k: wave = comb
    if (k < nchunks) {
      const int c0 = k * RV_CHUNK, cl = min(RV_CHUNK, live - c0);
      float* __restrict__ ln = line[wave];
      float* __restrict__ out = co[wave];
      int j = 0, p = c0 % D;
      while (j < cl) {
        const int seg = min(D - p, cl - j);
        for (int t = 0; t < seg; t += 64) {
          const int cnt = min(seg - t, 64), i = t + lane;
          const bool on = lane < cnt;
          const float o = on ? ln[p + i] : 0.0f;
          if (on) out[j + i] = o;
          float b = fmaf(-o, damp, o);
          if (cnt > 1) b = fmaf(d1, rv_row_shr<1>(b), b);
          if (cnt > 2) b = fmaf(d2, rv_row_shr<2>(b), b);
          if (cnt > 4) b = fmaf(d4, rv_row_shr<4>(b), b);
          if (cnt > 8) b = fmaf(d8, rv_row_shr<8>(b), b);
          float carry = store;                               // the state in front of this lane's row
          if (cnt > 16) {
            const float s1 = fmaf(d16, store, rv_lane(b, 15)), s2 = fmaf(d16, s1, rv_lane(b, 31)), s3 = fmaf(d16, s2, rv_lane(b, 47));
            carry = row == 0 ? store : row == 1 ? s1 : row == 2 ? s2 : s3;
          }
          const float s = fmaf(dlane, carry, b);
          if (on) ln[p + i] = fmaf(s, feedback, xs[j + i]);
          store = rv_lane(s, cnt - 1);
        }
        rv_wave_sync();
        j += seg;
        p += seg;
        if (p == D) p = 0;
      }
    }
    // ---- all-pass stage aps on chunk k - 1 - aps, in place: the cascade as a pipeline over chunks
    const int q = k - 1 - aps;
    if (wave < 2 * RV_AP_STAGES && q >= 0 && q < nchunks) {
      const int c0 = q * RV_CHUNK, cl = min(RV_CHUNK, live - c0);
      float* __restrict__ v = ap[apw][q % RV_AP_SLOTS];
      int j = 0, p = c0 % Da;
      while (j < cl) {
        const int seg = min(Da - p, cl - j);
        for (int i = lane; i < seg; i += 64) {
          const float o = aline[p + i], in = v[j + i];
          aline[p + i] = fmaf(0.5f, o, in);
          v[j + i] = o - in;
        }
        rv_wave_sync();
        j += seg;
        p += seg;
        if (p == Da) p = 0;
      }
    }
    __syncthreads();

    // ---- the comb sum of chunk k, 7 down to 0, into the chunk's slot
    if (k < nchunks) {
      const int w = tid / RV_CHUNK, j = tid % RV_CHUNK;
      float acc = 0.0f;
#pragma unroll
      for (int i = 7; i >= 0; --i) acc += co[w * 8 + i][j];
      ap[w][k % RV_AP_SLOTS][j] = acc;
    }
    // ---- out: chunk k - 4 has left the last all-pass
    const int qo = k - RV_AP_STAGES;
    if (qo >= 0 && tid < RV_CHUNK && qo * RV_CHUNK + tid < N_out) {
      const int n = qo * RV_CHUNK + tid;
      float o = 0.0f;
      if (n < live) {
        const float d = dry_gain * x[n];
        o = 0.5f * (fmaf(ap[0][qo % RV_AP_SLOTS][tid], wet_gain, d) + fmaf(ap[1][qo % RV_AP_SLOTS][tid], wet_gain, d));
      }
      y[n] = o;
    }
    // ---- the source of chunk k + 1
    if (k + 1 < nchunks && tid < RV_CHUNK) {
      const int n = (k + 1) * RV_CHUNK + tid;
      xs[tid] = n < live ? x[n] : 0.0f;
    }
    __syncthreads();
  }
  const int done = (live + RV_CHUNK - 1) / RV_CHUNK * RV_CHUNK;
  for (int n = done + tid; n < N_out; n += RV_THREADS) y[n] = 0.0f;
}

bool rv_buf_ok(const void* p, int64_t ld, int N) { return p && N >= 1 && N <= (1 << 30) && ld >= N; }

}  // namespace

extern "C" int w2v2_aug_reverb_chunk(void) { return RV_CHUNK; }

extern "C" int w2v2_aug_reverb(const float* src, int64_t ld_src, int N_in, const int32_t* lens, const int32_t* src_rows,
                               float* dst, int64_t ld_dst, int N_out, const int32_t* dst_rows, int R, const int32_t* params,
                               void* stream) {
  W2V2_REQUIRE(rv_buf_ok(src, ld_src, N_in) && rv_buf_ok(dst, ld_dst, N_out) && src_rows && dst_rows && R >= 1 && R <= 65535,
               "aug_reverb: bad arguments (src [rows][ld_src >= N_in >= 1], dst [rows][ld_dst >= N_out >= 1], two row lists of "
               "1..65535 entries)");
  W2V2_REQUIRE(src != dst, "aug_reverb: src and dst must not be the same buffer");
  W2V2_REQUIRE(params, "aug_reverb: params [R][%d] must be set", W2V2_AUG_REVERB_PARAMS);
  hipLaunchKernelGGL(aug_reverb_kernel, dim3((unsigned)R), dim3(RV_THREADS), 0, as_stream(stream), src, ld_src, N_in, lens,
                     src_rows, dst, ld_dst, N_out, dst_rows, params);
  W2V2_CHECK_LAUNCH("aug_reverb");
  return 0;
}
