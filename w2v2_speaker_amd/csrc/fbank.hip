// Log-mel filterbank front-end of the ECAPA-TDNN path on the device: the arithmetic of data/fbank.py (centred 400-point
// STFT under the periodic Hamming window, hop 160, power spectrum, mel product, 10 log10(max(., 1e-10)), clamp at 80 dB
// below the utterance's maximum) followed by InputNormalizer2D(normalize_over_channels=True) (data/pipeline.py).
//
// Two kernels.  fbank_db_kernel: one workgroup per (utterance, tile of FB_TILE frames) stages the windowed frames of its
// tile in LDS, takes a direct 400-tap DFT of bins 0..200 on the vector ALU (thread = bin, the 16 frames of the tile in
// registers; twiddles from a 400-entry table indexed by (j k) mod 400, never a sine of a large argument), writes the
// power spectrum over the staged frames, multiplies by the mel matrix and writes the dB values and the tile's maximum.
// fbank_normalize_kernel: one workgroup per (utterance, 8 mel channels) folds the tile maxima of the utterance, clamps,
// and normalises each channel with a two-pass mean / unbiased deviation in f64 accumulators.
//
// Variable lengths: every value of frame t of utterance b is a function of that utterance's own samples [0, n_b) alone
// -- taps are masked by INDEX, the tiles start at multiples of FB_TILE frames of the utterance, and the cross-frame
// reductions run over t < F_b in an order fixed by F_b (maximum: per tile, then over the tiles; column sums: row lane r
// of 128 takes frames t = r mod 128 in ascending order, then the 128 partial sums in ascending r).  Nothing depends on B, T,
// N or the grid, so rows t < F_b are bit-identical to the call on the utterance alone (B = 1, N = n_b).
#include "common.h"

namespace {

constexpr int FB_NFFT = 400;            // = window length (asserted on the host against data/fbank.py)
constexpr int FB_HOP = 160;
constexpr int FB_BINS = FB_NFFT / 2 + 1;
constexpr int FB_TILE = W2V2_FBANK_TILE_FRAMES;
constexpr int FB_PLD = 204;             // row stride of the power spectrum image (floats)
constexpr int FB_THREADS = 256;
static_assert(FB_TILE == 16, "fbank_db_kernel keeps the 16 frames of a tile in registers as four float4");
static_assert(FB_TILE * FB_PLD <= FB_NFFT * FB_TILE, "the power spectrum image reuses the staged frames' LDS");
static_assert(FB_BINS <= FB_THREADS, "one thread per bin");

// cos(2 pi i / 400), i = 0..100, computed on the host in f64 and rounded to f32; the kernel unfolds the full circle
// by the exact symmetries of the cosine (the kernel argument is 404 bytes instead of a table in device memory)
struct FbankQuarter { float c[FB_NFFT / 4 + 1]; };

__device__ __forceinline__ float fb_cos(const FbankQuarter& q, int i) {      // i in [0, 400)
  if (i <= 100) return q.c[i];
  if (i <= 200) return -q.c[200 - i];
  if (i <= 300) return -q.c[i - 200];
  return q.c[400 - i];
}

__global__ __launch_bounds__(FB_THREADS) void fbank_db_kernel(const float* __restrict__ wav, const int* __restrict__ lens,
                                                              const float* __restrict__ window,
                                                              const float* __restrict__ fbank, float* __restrict__ db,
                                                              float* __restrict__ pmax, const FbankQuarter q, int N,
                                                              int T, int n_mels, int ntile) {
  __shared__ float4 xs4[FB_NFFT * FB_TILE / 4];     // staged frames [tap j][frame f]; later the power image [f][FB_PLD]
  __shared__ float2 tw[FB_NFFT];                    // (cos, sin)(2 pi i / 400)
  __shared__ float red[FB_THREADS / 64];
  float* xs = reinterpret_cast<float*>(xs4);
  const int tid = threadIdx.x, b = blockIdx.y, tile = blockIdx.x, t0 = tile * FB_TILE;
  const int n = lens ? min(max(lens[b], 0), N) : N;
  const int F = 1 + n / FB_HOP;
  const float* w = wav + (int64_t)b * N;
  float* dbb = db + (int64_t)b * T * n_mels;

  if (t0 >= F) {                                    // (workgroup-uniform) a tile past the utterance: defined, unused values
    for (int it = tid; it < FB_TILE * n_mels; it += FB_THREADS) {
      const int t = t0 + it / n_mels;
      if (t < T) dbb[(int64_t)t * n_mels + it % n_mels] = 0.0f;
    }
    if (tid == 0) pmax[(int64_t)b * ntile + tile] = -INFINITY;
    return;
  }

  for (int i = tid; i < FB_NFFT; i += FB_THREADS) tw[i] = make_float2(fb_cos(q, i), fb_cos(q, (i + 300) % FB_NFFT));
  for (int idx = tid; idx < FB_NFFT * FB_TILE; idx += FB_THREADS) {
    const int f = idx / FB_NFFT, j = idx - f * FB_NFFT, t = t0 + f;
    const int64_t s = (int64_t)FB_HOP * t - FB_NFFT / 2 + j;
    float v = 0.0f;
    if (t < F && s >= 0 && s < n) v = w[s] * window[j];
    xs[j * FB_TILE + f] = v;
  }
  __syncthreads();

  const int k = tid;
  float re[FB_TILE], im[FB_TILE];
#pragma unroll
  for (int f = 0; f < FB_TILE; ++f) re[f] = im[f] = 0.0f;
  if (k < FB_BINS) {
    int ph = 0;                                     // (j k) mod 400
    for (int j = 0; j < FB_NFFT; ++j) {
      const float2 cs = tw[ph];
      ph += k;
      if (ph >= FB_NFFT) ph -= FB_NFFT;
      float x[FB_TILE];
#pragma unroll
      for (int g = 0; g < FB_TILE / 4; ++g) {
        const float4 v = xs4[j * (FB_TILE / 4) + g];
        x[4 * g] = v.x; x[4 * g + 1] = v.y; x[4 * g + 2] = v.z; x[4 * g + 3] = v.w;
      }
#pragma unroll
      for (int f = 0; f < FB_TILE; ++f) {
        re[f] = fmaf(x[f], cs.x, re[f]);
        im[f] = fmaf(x[f], cs.y, im[f]);
      }
    }
  }
  __syncthreads();                                  // every read of the staged frames is done: the image takes their place
  float* ps = xs;
  if (k < FB_BINS) {
#pragma unroll
    for (int f = 0; f < FB_TILE; ++f) ps[f * FB_PLD + k] = re[f] * re[f] + im[f] * im[f];
  }
  __syncthreads();

  float lmax = -INFINITY;
  for (int it = tid; it < FB_TILE * n_mels; it += FB_THREADS) {
    const int f = it / n_mels, m = it - f * n_mels, t = t0 + f;
    float acc = 0.0f;
    for (int kk = 0; kk < FB_BINS; ++kk) acc = fmaf(ps[f * FB_PLD + kk], fbank[kk * n_mels + m], acc);
    const float d = 10.0f * log10f(fmaxf(acc, 1e-10f));
    if (t < F) {
      dbb[(int64_t)t * n_mels + m] = d;
      lmax = fmaxf(lmax, d);
    } else if (t < T) {
      dbb[(int64_t)t * n_mels + m] = 0.0f;
    }
  }
  lmax = wave_max(lmax);
  if ((tid & 63) == 0) red[tid >> 6] = lmax;
  __syncthreads();
  if (tid == 0) {
    float v = red[0];
#pragma unroll
    for (int i = 1; i < FB_THREADS / 64; ++i) v = fmaxf(v, red[i]);
    pmax[(int64_t)b * ntile + tile] = v;
  }
}

// 1024 threads = 128 row lanes x 8 channels: one 145 s utterance (14501 frames) is 5 workgroups, and the three passes
// over its frames are chains of dependent loads -- 114 per thread instead of 454 with 256 threads (measured: 164 -> 60 us)
constexpr int FN_THREADS = 1024, FN_COLS = 8, FN_ROWS = FN_THREADS / FN_COLS;

template <typename TO>
__global__ __launch_bounds__(FN_THREADS) void fbank_normalize_kernel(const float* __restrict__ db,
                                                                     const float* __restrict__ pmax,
                                                                     const int* __restrict__ lens, TO* __restrict__ out,
                                                                     int64_t ldo, int T, int n_mels, int ntile) {
  __shared__ double part[FN_ROWS][FN_COLS];
  __shared__ double s_mean[FN_COLS];
  __shared__ float s_meanf[FN_COLS], s_den[FN_COLS], red[FN_THREADS / 64];
  const int tid = threadIdx.x, b = blockIdx.y, c = tid % FN_COLS, r = tid / FN_COLS, m = blockIdx.x * FN_COLS + c;
  const int F = lens ? min(1 + max(lens[b], 0) / FB_HOP, T) : T;
  const int nt = (F + FB_TILE - 1) / FB_TILE;
  const bool on = m < n_mels;
  const float* col = db + (int64_t)b * T * n_mels + m;
  TO* o = out + (int64_t)b * T * ldo + m;

  float gmax = -INFINITY;
  for (int i = tid; i < nt; i += FN_THREADS) gmax = fmaxf(gmax, pmax[(int64_t)b * ntile + i]);
  gmax = wave_max(gmax);
  if ((tid & 63) == 0) red[tid >> 6] = gmax;
  __syncthreads();
  gmax = red[0];
#pragma unroll
  for (int i = 1; i < FN_THREADS / 64; ++i) gmax = fmaxf(gmax, red[i]);
  const float lo = gmax - 80.0f;

  double s = 0.0;
  if (on)
    for (int t = r; t < F; t += FN_ROWS) s += (double)fmaxf(col[(int64_t)t * n_mels], lo);
  part[r][c] = s;
  __syncthreads();
  if (tid < FN_COLS) {
    double tot = 0.0;
    for (int i = 0; i < FN_ROWS; ++i) tot += part[i][tid];
    s_mean[tid] = tot / (double)F;
    s_meanf[tid] = (float)s_mean[tid];
  }
  __syncthreads();
  const double mean = s_mean[c];
  s = 0.0;
  if (on)
    for (int t = r; t < F; t += FN_ROWS) {
      const double d = (double)fmaxf(col[(int64_t)t * n_mels], lo) - mean;
      s += d * d;
    }
  part[r][c] = s;
  __syncthreads();
  if (tid < FN_COLS) {
    double tot = 0.0;
    for (int i = 0; i < FN_ROWS; ++i) tot += part[i][tid];
    s_den[tid] = (float)sqrt(tot / (double)(F - 1)) + 1e-5f;      // unbiased; one frame: 0 / 0, as torch.std
  }
  __syncthreads();
  if (!on) return;
  const float meanf = s_meanf[c], den = s_den[c];
  for (int t = r; t < F; t += FN_ROWS)
    o[(int64_t)t * ldo] = from_f32<TO>((fmaxf(col[(int64_t)t * n_mels], lo) - meanf) / den);
  for (int t = F + r; t < T; t += FN_ROWS) o[(int64_t)t * ldo] = from_f32<TO>(0.0f);
}

const FbankQuarter& fbank_quarter() {
  static const FbankQuarter q = [] {
    FbankQuarter v;
    for (int i = 0; i <= FB_NFFT / 4; ++i) v.c[i] = (float)cos(2.0 * 3.14159265358979323846 * (double)i / (double)FB_NFFT);
    return v;
  }();
  return q;
}

}  // namespace

extern "C" int w2v2_fbank_db(const float* wav, const int* lens, const float* window, const float* fbank, float* db_out,
                             float* partial_max, int B, int N, int T, int n_mels, void* stream) {
  W2V2_REQUIRE(wav && window && fbank && db_out && partial_max && B > 0 && B <= 65535 && N > 0 && n_mels > 0,
               "fbank_db: bad arguments (B %d, N %d, n_mels %d)", B, N, n_mels);
  W2V2_REQUIRE(T == 1 + N / FB_HOP, "fbank_db: T = %d, but %d samples give 1 + N / 160 = %d frames", T, N, 1 + N / FB_HOP);
  const int ntile = (int)cdiv(T, FB_TILE);
  hipLaunchKernelGGL(fbank_db_kernel, dim3((unsigned)ntile, (unsigned)B), dim3(FB_THREADS), 0, as_stream(stream), wav, lens,
                     window, fbank, db_out, partial_max, fbank_quarter(), N, T, n_mels, ntile);
  W2V2_CHECK_LAUNCH("fbank_db");
  return 0;
}

extern "C" int w2v2_fbank_normalize(const float* db, const float* partial_max, const int* lens, void* out, int64_t ldo,
                                    int dtype, int B, int T, int n_mels, void* stream) {
  W2V2_REQUIRE(db && partial_max && out && B > 0 && B <= 65535 && T > 0 && n_mels > 0 && ldo >= n_mels,
               "fbank_normalize: bad arguments (B %d, T %d, n_mels %d, ldo %lld)", B, T, n_mels, (long long)ldo);
  const int ntile = (int)cdiv(T, FB_TILE);
  const dim3 grid((unsigned)cdiv(n_mels, FN_COLS), (unsigned)B);
  switch (dtype) {
    case W2V2_F32:
      hipLaunchKernelGGL(fbank_normalize_kernel<float>, grid, dim3(FN_THREADS), 0, as_stream(stream), db, partial_max, lens,
                         (float*)out, ldo, T, n_mels, ntile);
      break;
    case W2V2_BF16:
      hipLaunchKernelGGL(fbank_normalize_kernel<bf16_t>, grid, dim3(FN_THREADS), 0, as_stream(stream), db, partial_max,
                         lens, (bf16_t*)out, ldo, T, n_mels, ntile);
      break;
    default: W2V2_FAIL("fbank_normalize: f32 or bf16 output (got dtype %d)", dtype);
  }
  W2V2_CHECK_LAUNCH("fbank_normalize");
  return 0;
}
