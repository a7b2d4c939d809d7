// wgrad_common.h -- what the four grouped weight-gradient kernels share (wgrad.hip: 128x128 two-stage, 256x128 ring and
// 256x256x32 ring; wgrad_phased.hip: 256x256x64 phased).  Each kernel keeps its staging, its schedule and its wave map;
// everything else is here or in common.h:
//   WgProblem / WgArgs   the kernel-argument block (one entry per (dY, X) pair of the launch)
//   wg_f                 the segment swizzle of the K-major LDS images
//   WG_PROBLEM_OF_TILE   tile -> problem (the tile itself comes from xcd_remap, common.h)
//   wg_dbias_add         dbias partial sums from a dY fragment that is in registers anyway
//   WG_DBIAS_STORE       ... summed over the four lane groups and stored
//   WG_STORE_ROWS        LDS -> HBM half of the coalesced f32 tile store
//   common.h             TrFrag / tr_read / landed (transposing fragment reads), wait_vmcnt / wait_pieces / wait_quarters
#pragma once
#include "common.h"
#include <stdlib.h>

constexpr int WG_MAXP = 32;

struct WgProblem {
  const bf16_t* dY;
  const bf16_t* X;
  float* dW;
  float* dbias;
  int64_t ld_dy, ld_x, ld_dw;
  int n_out, n_in;
  int tile_begin, tiles_n;
};
struct WgArgs {
  WgProblem p[WG_MAXP];
  int n_problems, total_tiles, ktiles;
};

// The 32-byte segments of a token row are XOR-swizzled with f(r), r = token row -- on the DMA source address and again on
// the read: the 8 rows a half-wave's transposing read touches land on 8 different segments (conflict-free).
__device__ __forceinline__ int wg_f(int r) { return (r & 3) | ((r >> 1) & 4); }

// The three pieces below that read the problem block are MACROS on purpose.  The block sits in kernel-argument memory and the
// kernels index it with a run-time problem number; as soon as a function -- force-inlined, taking WgArgs or WgProblem by
// reference or by pointer, or their fields by value -- stands between the kernel and those loads, the compiler places them
// differently, and with them the registers of the K loop in front (profiles/shared_pieces_device_code.txt).  Expanded in
// the kernel they compile to the instruction streams the kernels had with private copies.
//
// `const WgProblem& P` = the problem that owns `tile` (tile_begin ascends)
#define WG_PROBLEM_OF_TILE(P, a, tile)                                          \
  int wg_pi_ = 0;                                                               \
  _Pragma("unroll") for (int i = 1; i < WG_MAXP; ++i)                           \
    if (i < (a).n_problems && (tile) >= (a).p[i].tile_begin) wg_pi_ = i;        \
  const WgProblem& P = (a).p[wg_pi_]

// dbias[m] = sum_t dY[t][m]: the waves that own n-tile 0 add up the dY fragments they hold anyway, two values per
// v_dot2c_f32_{bf16,f16} against (1, 1) = ones_pair<TE>() -- 4 VALU ops per fragment instead of 16 converts + adds
template <typename TE> __device__ __forceinline__ float wg_dbias_add(frag8_t dy, uint32_t one2, float s) {
  union { frag8_t v; uint32_t p[4]; } u;
  u.v = dy;
#pragma unroll
  for (int e = 0; e < 4; ++e) s = pair_sum_add<TE>(u.p[e], one2, s);
  return s;
}
// a lane's sum covers the k-slots of its lane group: add the four groups, lanes 0..15 store row m (m includes lane & 15)
#define WG_DBIAS_STORE(P, sum, m_, lane)                                        \
  {                                                                             \
    float s = (sum);                                                            \
    s += __shfl_xor(s, 16, 64);                                                 \
    s += __shfl_xor(s, 32, 64);                                                 \
    const int m = (m_);                                                         \
    if (((lane) >> 4) == 0 && m < (P).n_out) (P).dbias[m] = s;                  \
  }

// Coalesced f32 tile store through LDS, second half: ROWS rows of the tile staged as f32 [ROWS][BN + 4] (the accumulator
// -> LDS half follows the kernel's wave map and stays there) go out as 16-byte write-through stores, BN / 4 lanes per
// row.  NT = threads of the workgroup; mbase = first row, n0 = first column of the staged rows in dW.
#define WG_STORE_ROWS(NT, ROWS, BN, P, stagef, mbase, n0, tid)                                                             \
  _Pragma("unroll") for (int it = 0; it < (ROWS) * ((BN) / 4) / (NT); ++it) {                                              \
    const int c = (tid) + (NT) * it;                                                                                       \
    const int r = c >> __builtin_ctz((BN) / 4), ch = c & ((BN) / 4 - 1);                                                   \
    const int m = (mbase) + r, n = (n0) + ch * 4;                                                                          \
    if (m < (P).n_out && n + 4 <= (P).n_in)                                                                                \
      store16_wt((P).dW + (int64_t)m * (P).ld_dw + n, *reinterpret_cast<const uint4*>((stagef) + r * ((BN) + 4) + ch * 4)); \
  }

// wgrad_phased.hip: the 256x256x64 phased kernel; `dtype` = W2V2_BF16 / W2V2_F16, one workgroup per tile
// late = DMA pieces of a phase (0..2) issued between its MFMAs; != 0: the launch could not be prepared
int w2v2_launch_wgrad_phased(const WgArgs& a, int dtype, int tiles, int late, hipStream_t st);
