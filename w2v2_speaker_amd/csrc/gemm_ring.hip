// gemm_ring.hip -- 256x128x64 three-stage LDS-DMA ring GEMM (see gemm_common.h for the family map).
#include "gemm_common.h"

// ------------------------------------------------------------------------------ 256x128x64, 3-stage LDS-DMA ring
// The 128x128 kernel moves 32 KiB from L2 per 2.1 MFLOP (64 FLOP/B): at 2 workgroups per CU that is a
// large fraction of the aggregate L2 bandwidth, and its 1-tile prefetch distance (vmcnt(0) before every
// barrier) exposes the L2/HBM latency once per K tile.  This variant uses a 256x128 block tile (8 waves
// as 4x2, 64x64 per wave, 87 FLOP/B) and a 3-stage LDS ring (144 KiB) with a COUNTED wait: while tile t
// is multiplied, tiles t+1 and t+2 are in flight; per K tile one raw s_barrier and `s_waitcnt vmcnt(G)`
// (G = this wave's DMA pieces per stage), never vmcnt(0) in the loop.
template <typename TE, typename TC, bool DBG = false>
__global__ __launch_bounds__(512) void gemm16_ring_256x128_kernel(const GemmArgs g) {
  constexpr int BM = 256, BN = 128, FM = 4, FN = 4;
  constexpr int STAGE = (BM + BN) * 64;           // elements per stage (A then B)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  bf16_t* smem = reinterpret_cast<bf16_t*>(smem_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // 0..7
  const int wm = wave >> 1, wn = wave & 1;

  // Deferred stores (g.defer_ok): the 8 x 16-byte stores of a tile are kept packed in registers and issued in the
  // first three ring steps of the NEXT tile (ahead of that step's DMA pieces, so the counted vmcnt waits stay valid):
  // issued together at the tile end they leave at the HBM write rate (~9 B/clk per CU) while nothing else runs.
  uint4 pend[8];
  bool pending = false;
  int pend_m = 0, pend_n = 0;
  TC* const Cdef = reinterpret_cast<TC*>(g.C) + (blockIdx.z / g.batch_inner) * g.c_s0 +
                   (blockIdx.z % g.batch_inner) * g.c_s1;
  // pend[2 i], pend[2 i + 1] = rows pend_m + 16 i and + 8, columns pend_n .. pend_n + 7 (epilogue_lines)
  auto flush = [&](auto first, auto count) {
    if constexpr (sizeof(TC) == 2) {
#pragma unroll
      for (int q = decltype(first)::value; q < decltype(first)::value + decltype(count)::value; ++q) {
        const int mi = pend_m + 16 * (q >> 1) + 8 * (q & 1);
        if (mi < g.M) {
          if (g.wt_stores) store16_wt(Cdef + (int64_t)mi * g.ldc + pend_n, pend[q]);
          else *reinterpret_cast<uint4*>(Cdef + (int64_t)mi * g.ldc + pend_n) = pend[q];
        }
      }
    }
  };
  // Persistent over tiles: gridDim.x = min(tiles, CUs) workgroups, each takes tiles t, t + G, ...  (one 144 KiB
  // workgroup per CU anyway).  The tiles of a workgroup are ONE K stream through the ring: K tile kt of a tile lives in
  // stage (phase + kt) % 3 where `phase` runs on from the previous tile, the last two ring steps of a tile (which have
  // nothing of their own left to request) request K tiles 0 and 1 of the NEXT tile, and that tile enters its loop on
  // the counted wait -- no barrier and no prologue between tiles: the operands land under the epilogue.  (Measured in
  // the step, A B A B A B on one box: 10.15 -> 9.99 ms, profiles/stream_tiles_ab.txt.)
  const int ntile = g.tiles_m * g.tiles_n;
  const int G = gridDim.x;
  const int z = blockIdx.z;
  const int z0 = z / g.batch_inner, z1 = z - z0 * g.batch_inner;
  // K steps of a tile: nk1 over (A, B) + for the tiles of the two-term weight columns nk - nk1 more over (A, B_lo)
  const int nk1 = g.K >> 6;
  auto tile_nk = [&](int n0) -> int { return nk1 + ((g.k_ext > 0 && n0 >= g.n_ext_from) ? (g.k_ext >> 6) : 0); };
  auto koff_a = [&](int kt) -> int { return (kt < nk1 ? kt : kt - nk1) * 64; };
  auto koff_b = [&](int kt) -> int64_t { return kt < nk1 ? (int64_t)kt * 64 : (int64_t)(kt - nk1) * 64 + g.b_lo_off; };

  const bf16_t* Ab = reinterpret_cast<const bf16_t*>(g.A.ptr) + z0 * g.a_s0 + z1 * g.a_s1;
  const bf16_t* Bb = reinterpret_cast<const bf16_t*>(g.B.ptr) + z0 * g.b_s0 + z1 * g.b_s1;

  // per-lane sources of this wave's DMA pieces (gemm_common.h: ring_tile_srcs).  They belong to the tile whose operands
  // are being requested: the current one until its last K tile has been requested, then the NEXT one
  const bf16_t* ap[4];
  const bf16_t* bp[2];

  f32x4 acc[FM][FN];

  auto stage = [&](bf16_t* base, int kt) {
    bf16_t* ad = base + wave * 4 * 8 * 64;
    bf16_t* bd = base + BM * 64 + wave * 2 * 8 * 64;
    const int ka = koff_a(kt);
    const int64_t kb = koff_b(kt);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      w2v2_dma16((ap[j] + ka), (ad + j * 8 * 64));
#pragma unroll
    for (int j = 0; j < 2; ++j)
      w2v2_dma16((bp[j] + kb), (bd + j * 8 * 64));
  };
  const int frow = lane & 15, fk = lane >> 4;
  // per-lane fragment offsets (elements) for k-step 0 / 1; everything else is a compile-time constant
  const int lo0 = frow * 64 + ((fk ^ swz(frow)) << 3);
  const int lo1 = frow * 64 + (((4 + fk) ^ swz(frow)) << 3);
  // B fragment j, operand row rho = frow  <->  tile row (rho >> 2) * 16 + j * 4 + (rho & 3): after the MFMA a lane
  // owns the 16 CONSECUTIVE columns fk * 16 + j * 4 + e of its row (register epilogue below)
  const int brow = (frow >> 2) * 16 + (frow & 3);
  const int lb0 = brow * 64 + ((fk ^ swz(frow)) << 3);
  const int lb1 = brow * 64 + (((4 + fk) ^ swz(frow)) << 3);
  const int aoff = wm * 64 * 64, boff = BM * 64 + wn * 64 * 64;
  // piece p of the 6 DMA pieces of one stage: A0..A3, B0, B1
  auto stage_piece = [&](bf16_t* base, int kt, int p) {
    if (p < 4)
      w2v2_dma16((ap[p] + koff_a(kt)), (base + (wave * 4 + p) * 8 * 64));
    else
      w2v2_dma16((bp[p - 4] + koff_b(kt)), (base + BM * 64 + (wave * 2 + p - 4) * 8 * 64));
  };
  // multiply stage `base`; when kload >= 0 the DMA pieces of K tile kload go to `nxt`, spread over the MFMA groups
  // (issued back to back behind the barrier they keep both waves of a SIMD in the queue-limited DMA issue)
  // tools only (w2v2_tune_gemm_ring_debug -> g.dbg_bits, read by the DBG instantiation alone; results are garbage):
  //   1 = no DMA pieces in the steady-state loop, 2 = no barrier in the loop, 4 = no vmcnt wait in the loop, 8 = no fragment reads
  const int dbg = DBG ? g.dbg_bits : 0;
  auto compute = [&](const bf16_t* base, bf16_t* nxt, int kload) {
    if (dbg & 1) kload = -1;
    const bf16_t* a0 = base + aoff + lo0;
    const bf16_t* a1 = base + aoff + lo1;
    const bf16_t* b0 = base + boff + lb0;
    const bf16_t* b1 = base + boff + lb1;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      frag8_t af[FM], bfr[FN];
      if (DBG && (dbg & 8)) {                      // registers as they are (no load, nothing kept live for it)
#pragma unroll
        for (int i = 0; i < FM; ++i) asm volatile("" : "=v"(af[i]));
#pragma unroll
        for (int j = 0; j < FN; ++j) asm volatile("" : "=v"(bfr[j]));
      } else {
#pragma unroll
        for (int i = 0; i < FM; ++i) af[i] = *reinterpret_cast<const frag8_t*>((kk ? a1 : a0) + i * 16 * 64);
#pragma unroll
        for (int j = 0; j < FN; ++j) bfr[j] = *reinterpret_cast<const frag8_t*>((kk ? b1 : b0) + j * 4 * 64);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = mfma16<TE>(bfr[j], af[i], acc[i][j]);
        if (kload >= 0) {
          __builtin_amdgcn_sched_barrier(0);
          if (kk == 0) {
            stage_piece(nxt, kload, i);                  // pieces 0..3 behind the four groups of the first half
          } else if (i < 2) {
            stage_piece(nxt, kload, 4 + i);              // pieces 4, 5
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  };
  // ---- the stream.  phase = ring stage of the K tile the next step multiplies; inflight = K tiles requested and not
  // yet waited for (1 or 2 at a step's wait: the one it multiplies and, mostly, the one behind it)
  int phase = 0, inflight = 0, kt = 0, nk = 0;
  // one ring step: K tile kt of the current tile is in stage `phase`; when kload >= 0, K tile kload of the tile ap / bp
  // point into goes to the stage two further on, which held the step before this one's and is free behind the barrier.
  // The counted wait holds whatever else the wave has in flight: vmcnt retires in order and every other operation
  // (deferred stores, an epilogue's loads) is OLDER than the newest K tile's six pieces or is drained explicitly.
  // Deferred stores of the previous tile ride on the first three steps, AHEAD of the step's DMA pieces: behind them
  // they would make the next step's vmcnt(6) wait for part of the K tile after next.
  auto step = [&](int kload) {
    if (!(dbg & 4)) { if (inflight > 1) wait_vmcnt<6>(); else wait_vmcnt<0>(); }
    --inflight;
    if (!(dbg & 2)) __builtin_amdgcn_s_barrier();
    if (pending) {                                         // (only where nk >= 3: shorter tiles flush in one piece)
      if (kt == 0) flush(std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{});
      else if (kt == 1) flush(std::integral_constant<int, 3>{}, std::integral_constant<int, 3>{});
      else { flush(std::integral_constant<int, 6>{}, std::integral_constant<int, 2>{}); pending = false; }
    }
    compute(smem + phase * STAGE, smem + (phase == 0 ? 2 : phase - 1) * STAGE, kload);
    if (kload >= 0) ++inflight;
    phase = phase == 2 ? 0 : phase + 1;
    ++kt;
  };

  int t0 = 0;
  int tile = persistent_tile(t0, ntile, G);
  if (tile < 0) return;
  int m0, n0;
  {
    int tm, tn;
    ring_tile_coords(g, tile, tm, tn);
    m0 = tm * BM;
    n0 = tn * BN;
  }
  nk = tile_nk(n0);
  ring_tile_srcs(g, Ab, Bb, m0, n0, wave, lane, ap, bp);
  int pre = 0;                           // K tiles of the current tile that the previous tile's last steps requested
  w2v2_vmcnt0_visible();                 // (common.h: keeps the compiler's own vmcnt(0) out of the loop)
#pragma unroll 1
  for (;;) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // K tiles 0 and 1 where no step has requested them (the first tile; the tile behind a one-step tile).  Their stages
    // held the K tiles three and two steps back: every wave has left those (this wave passed the last step's barrier).
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (j >= pre && j < nk) {
        const int sj = phase + j;
        stage(smem + (sj >= 3 ? sj - 3 : sj) * STAGE, j);
        ++inflight;
      }
    kt = 0;
    if (pending && nk < 3) {
      flush(std::integral_constant<int, 0>{}, std::integral_constant<int, 8>{});
      pending = false;
    }
    // steps that still have a K tile of their own tile to request
#pragma unroll 1
    while (kt + 2 < nk) step(kt + 2);
    // ---- the last two steps: the sources of this tile are dead, they become the next tile's (decode and addresses
    // cost ~600 dependent instructions: here they run while K tiles nk - 2 and nk - 1 are landing)
    t0 += G;
    tile = persistent_tile(t0, ntile, G);
    int m0n = 0, n0n = 0, nkn = 0;
    if (tile >= 0) {
      int tm, tn;
      ring_tile_coords(g, tile, tm, tn);
      m0n = tm * BM;
      n0n = tn * BN;
      nkn = tile_nk(n0n);
      ring_tile_srcs(g, Ab, Bb, m0n, n0n, wave, lane, ap, bp);
    }
    // (a one-step tile has no second step to request K tile 0 of the next tile from: that tile requests its own)
    const bool stream = tile >= 0 && nk >= 2;
#pragma unroll 1
    while (kt < nk) {
      const int j = kt + 2 - nk;
      step(stream && j < nkn ? j : -1);
    }
    pre = stream ? min(nkn, 2) : 0;

    // Register epilogue: thanks to the permuted B rows a lane holds, for each of its four rows, 16 consecutive
    // output columns (32 B of bf16): bias / GELU / residual are applied in registers and stored as 2 x 16 B per lane,
    // four lanes covering 128 contiguous bytes of a row -- no LDS round trip and no barrier after the main loop.
    if (DBG && (dbg & 32) && g.M > 0) {                  // (tools: no epilogue)
      asm volatile("" :: "v"(acc[0][0]), "v"(acc[3][3]));
    } else {
      TC* Cz = reinterpret_cast<TC*>(g.C) + z0 * g.c_s0 + z1 * g.c_s1;
      TC* auxz = g.aux ? reinterpret_cast<TC*>(g.aux) + z0 * g.aux_s0 + z1 * g.aux_s1 : nullptr;
      const float* bias = g.bias ? g.bias + z1 * g.bias_s1 : nullptr;
      const int nc = n0 + wn * 64 + fk * 16;
      float cv0[8], cv1[8];
      load_col8(g, bias, nc, cv0);
      load_col8(g, bias, nc + 8, cv1);
      if constexpr (sizeof(TC) == 2) {
        if (g.defer_ok) {            // (the host grants defer_ok only where lines_ok holds)
          W2V2_EPI_DISPATCH((epilogue_lines<TC, EPI, 4, true>(g, Cz, auxz, acc, m0 + wm * 64, nc, lane, cv0, cv1, pend)));
          pending = true;
          pend_m = m0 + wm * 64 + (frow & 7);
          pend_n = nc + (frow < 8 ? 0 : 8);
        } else if (lines_ok(g)) {
          W2V2_EPI_DISPATCH((epilogue_lines<TC, EPI, 4>(g, Cz, auxz, acc, m0 + wm * 64, nc, lane, cv0, cv1, pend)));
        } else {
          W2V2_EPI_DISPATCH((epilogue_direct<TC, EPI, 4>(g, Cz, auxz, acc, m0 + wm * 64 + frow, nc, cv0, cv1)));
        }
      } else {
        W2V2_EPI_DISPATCH((epilogue_direct<TC, EPI, 4>(g, Cz, auxz, acc, m0 + wm * 64 + frow, nc, cv0, cv1)));
      }
    }
    if (tile < 0) break;
    m0 = m0n;
    n0 = n0n;
    nk = nkn;
    // stores that were not deferred are drained here, as before; with deferred stores the stream runs on the counted
    // waits.  (The compiler still guards the registers of column operands an epilogue kind loaded without using them
    // with one vmcnt(0) of its own at the tile entry -- tools/loop_waits.sh shows it OUTSIDE both K loops: by then the
    // two requested stages have had the epilogue to land.)
    if (!pending) w2v2_vmcnt0_visible();
  }   // tile loop
  if (pending) flush(std::integral_constant<int, 0>{}, std::integral_constant<int, 8>{});
}

template <typename TE, typename TC, bool DBG>
static int launch_ring_v(GemmArgs a, int M, int N, int batch, bool persistent, hipStream_t st) {
  constexpr size_t lds = (size_t)3 * (256 + 128) * 64 * sizeof(bf16_t);   // 144 KiB
  a.tiles_m = (int)cdiv(M, 256);
  a.tiles_n = (int)cdiv(N, 128);
  const int ncu = persistent ? w2v2_gemm_device_cus() : (1 << 30);
  const int tiles = a.tiles_m * a.tiles_n;
  dim3 grid(tiles < ncu ? tiles : ncu, 1, batch);
  return w2v2_launch_lds<&gemm16_ring_256x128_kernel<TE, TC, DBG>, true>("gemm16_ring_256x128_kernel", grid, dim3(512), lds, st, a);
}

static int g_ring_dbg = 0;            // tools only: time-attribution variants of the ring kernel's K loop (garbage results)
extern "C" int w2v2_tune_gemm_ring_debug(int bits) {
  const int old = g_ring_dbg;
  g_ring_dbg = bits & 63;          // bit 4: the attribution kernel with nothing removed (its own baseline); bit 5: no epilogue
  return old;
}
template <typename TE, typename TC>
static int launch_ring(GemmArgs a, int M, int N, int batch, bool persistent, hipStream_t st) {
  if constexpr (std::is_same<TE, f16_t>::value && std::is_same<TC, f16_t>::value) {
    if (g_ring_dbg != 0) {                                  // tools: attribution variants, fp16 in / fp16 out only
      a.dbg_bits = g_ring_dbg;
      return launch_ring_v<f16_t, f16_t, true>(a, M, N, batch, persistent, st);
    }
  }
  return launch_ring_v<TE, TC, false>(a, M, N, batch, persistent, st);
}
int w2v2_launch_ring_256x128(const GemmArgs& a, int dtype_ab, int dtype_c, int M, int N, int batch, bool persistent,
                             hipStream_t st) {
  if (dtype_ab == W2V2_BF16)
    return dtype_c == W2V2_F32 ? launch_ring<bf16_t, float>(a, M, N, batch, persistent, st)
                               : launch_ring<bf16_t, bf16_t>(a, M, N, batch, persistent, st);
  return dtype_c == W2V2_F32 ? launch_ring<f16_t, float>(a, M, N, batch, persistent, st)
                             : launch_ring<f16_t, f16_t>(a, M, N, batch, persistent, st);
}
