"""GPU tests of the persistent 16-bit LDS-DMA GEMM kernels (csrc/gemm_ring.hip, csrc/gemm_phased.hip) where a workgroup
walks THREE OR MORE tiles, so that it crosses a tile boundary twice.  On the ring the operand stream runs across the
boundary: the last two ring steps of a tile request K tiles 0 and 1 of the workgroup's next tile, which land under the
epilogue, and the next tile enters its loop on the counted wait.  The phased kernel starts every tile from its own
prologue (streaming its quarters ahead of the epilogue measured slower, profiles/stream_tiles_ab.txt); its cases hold
the same walk to the same references.

Shapes follow the device's CU count n: 2 n < tiles <= 3 n (about 2.5 n, so that many workgroups own a third tile), and
one case with tiles = 2 n + 1, whose last round is a chunk of one tile (xcd_remap with nchunk < G).  Cases, float64
references and judging are those of tests/gemm_cases.py, launched as tests/test_gemm_edges_gpu.py launches them: every
case is of the EXACT class (every partial sum exact in f32), so an element multiplied from a wrong, stale or half-landed
stage differs from the reference bit for bit; only the GELU epilogue, which is not exact, takes the gelu class's bound.
NaN-prefilled guard rows and columns around C and aux catch a store outside the tile."""
import os

import pytest

import gemm_cases as GC
from test_gemm_edges_gpu import cus, run_all

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(any(os.environ.get(e) for e in GC.SWITCHES),
                                 reason="an A/B switch of the library moves products between kernels")]
AB = "f16"                                           # the type the benchmarked step runs in
RING_K = (64, 128, 192, 256, 320)                    # nk = 1 .. 5: below, at and above the ring depth of 3
PHASED_K = (64, 128, 192)
RING_COLS, PHASED_COLS = 3, 3                        # N = 384 (ring, 128-column tiles) / 768 (phased, 256-column tiles)


def stream_rows(n, cols, tiles=None, ragged=False):
    """M of a product of `cols` tile columns with about 2.5 n tiles (or exactly `tiles`): 256-row tiles."""
    tiles_m = (5 * n // 2) // cols + 1 if tiles is None else tiles // cols
    return 256 * tiles_m - (37 if ragged else 0)


def tiles_of(cs, bn):
    return -(-cs["M"] // 256) * (cs["N"] // bn)


def short_chunk_cols(n):
    """Tile columns c with c | 2 n + 1 (the product then has exactly 2 n + 1 tiles); 1 always does."""
    return next(c for c in (3, 5, 7, 9, 11, 13, 1) if (2 * n + 1) % c == 0)


def check_walk(cases, n, bn):
    for cs in cases:
        t = tiles_of(cs, bn)
        assert 2 * n < t <= 3 * n, (cs["name"], t, n)


@pytest.mark.parametrize("K", RING_K)
def test_ring_stream_over_three_tiles(K):
    """nk = 1 .. 5 on the ring: one-step tiles request nothing ahead (the next tile stages its own K tiles 0 and 1),
    two-step tiles request both from their only two steps, nk = 3 has one step of its own requests, nk >= 4 the steady
    loop.  The 16-bit C leaves its stores pending into the next tile (deferred), the f32 C does not (full drain)."""
    n = cus()
    M, N = stream_rows(n, RING_COLS), 128 * RING_COLS
    cases = [GC.forced("stream", 2, M, N, K, AB, AB), GC.forced("stream", 2, M, N, K, AB, "f32")]
    assert all(cs["fam"] == 2 for cs in cases)
    check_walk(cases, n, 128)
    run_all(cases, label=f" K={K}")


@pytest.mark.parametrize("K", RING_K)
def test_ring_stream_two_term_columns(K):
    """n_ext_from at the tile edge 128 of N = 384: the tiles of the last two tile columns run 2 nk K steps and are
    enumerated first, so a workgroup's consecutive tiles differ in nk (2 nk, then nk) -- the tile that requests ahead
    has to ask for the NEXT tile's count of K tiles, not its own."""
    n = cus()
    M, N = stream_rows(n, RING_COLS), 128 * RING_COLS
    cases = [GC.case("stream two-term", 2, M, N, K, AB, AB, n_ext_from=128)]
    check_walk(cases, n, 128)
    run_all(cases, label=f" K={K}")


def test_ring_stream_epilogues_batch_and_ragged_rows():
    """BIAS and ADD (aux read in place) with deferred stores, MUL without (defer_ok off, whole lines), two products on
    the batch axis, and a last row tile that is partly filled; K = 192 and 256: the deferred stores ride on the first
    three steps of a tile, which are also the ones that request ahead at nk = 3."""
    n = cus()
    M, N = stream_rows(n, RING_COLS), 128 * RING_COLS
    Mr = stream_rows(n, RING_COLS, ragged=True)
    cases = [GC.forced("stream", 2, M, N, 192, AB, AB, epi="bias"),
             GC.forced("stream", 2, M, N, 192, AB, AB, epi="add", aux_is_c=True),
             GC.forced("stream", 2, M, N, 256, AB, AB, epi="mul"),
             GC.forced("stream", 2, Mr, N, 256, AB, AB, epi="bias"),
             # (the tuner moves single products only: a batched one reaches the ring on the default route, N >= 512)
             GC.case("stream", 2, stream_rows(n, 4), 512, 192, AB, AB, batch=(1, 2))]
    assert all(cs["fam"] == 2 for cs in cases)
    check_walk(cases, n, 128)                        # (batched: every product of the batch walks its own tiles)
    run_all(cases)


def test_ring_stream_short_last_chunk():
    """tiles = 2 n + 1: the third round is a chunk of ONE tile, remapped with nchunk = 1 < G, and every other workgroup
    finds no next tile in its second one."""
    n = cus()
    cols = short_chunk_cols(n)
    M, N = stream_rows(n, cols, tiles=2 * n + 1), 128 * cols
    cases = [GC.forced("stream 2n+1", 2, M, N, 192, AB, AB), GC.forced("stream 2n+1", 2, M, N, 128, AB, AB, epi="bias")]
    assert all(tiles_of(cs, 128) == 2 * n + 1 and cs["fam"] == 2 for cs in cases)
    run_all(cases)


@pytest.mark.parametrize("K", PHASED_K)
def test_phased_stream_over_three_tiles(K):
    """nk = 1, 2, 3 on the phased kernel over three tiles per workgroup: each tile's six prologue quarters refill both
    K-tile buffers behind the previous tile's catch-up barrier and epilogue (16-bit whole lines and the f32 per-lane
    form)."""
    n = cus()
    M, N = stream_rows(n, PHASED_COLS), 256 * PHASED_COLS
    cases = [GC.forced("stream", 4, M, N, K, AB, AB), GC.forced("stream", 4, M, N, K, AB, "f32", epi="bias")]
    assert all(cs["fam"] == 4 for cs in cases)
    check_walk(cases, n, 256)
    run_all(cases, label=f" K={K}")


def test_phased_stream_bias_gelu_writes_aux_and_short_last_chunk():
    """ADD (aux read in place) over about 2.5 n tiles, and BIAS_GELU (C and a written aux) with tiles = 2 n + 1, the
    fewest the walk allows: the gelu class's reference is the costly one."""
    n = cus()
    M, N = stream_rows(n, PHASED_COLS), 256 * PHASED_COLS
    cols = short_chunk_cols(n)
    cases = [GC.forced("stream", 4, M, N, 64, AB, AB, epi="add", aux_is_c=True),
             GC.forced("stream 2n+1", 4, stream_rows(n, cols, tiles=2 * n + 1), 256 * cols, 128, AB, AB, "gelu", "bias_gelu",
                       alpha=2.0 ** -5)]
    assert all(cs["fam"] == 4 for cs in cases)
    check_walk(cases[:1], n, 256)
    assert tiles_of(cases[1], 256) == 2 * n + 1
    run_all(cases)
