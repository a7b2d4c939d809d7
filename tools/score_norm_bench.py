"""Timing of the device score normalisation (csrc/score_norm.hip + the exact-f32 GEMM) at the size of a VoxCeleb
evaluation: N = 145,160 bank rows, M = 5,994 cohort rows (one per training speaker), K = 300, P = 579,818 trials
(VoxCeleb1-E), D = 192 and 1,536.  Per D, with HIP events around each stage of ops.cohort_stats' own block loop, summed
over the blocks of one pass and reported as the median of --reps passes after one warm-up pass:
  transform   w2v2_rows_transform of the cohort and of every bank block (centring + length norm on, so that it copies)
  product     S_block = U_block C^T (ops.Gemm, EPI_SCALE_RC), against the sustained f32 matrix-pipe rate
  topk_stats  w2v2_topk_stats of every block, against the bytes of S it reads
  trial pass  w2v2_score_pairs + w2v2_score_pairs_norm over the P trials
and next to them the same computation in torch on the same device, in the same process and with the same blocks:
normalised matmul + topk + mean / std.  No time target is asserted; the file records what came out.
    python tools/score_norm_bench.py [--reps 5] [--out profiles/score_norm_bench.txt]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from w2v2_speaker_amd import ops

dev = "cuda"
N, M, K, P = 145160, 5994, 300, 579818
F32_MATRIX_TFLOPS = 153.7      # profiles/r05_mfma_f32_sustained.txt (tools/probes/mfma_f32_sustained_probe.hip)
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


class Stage:
    """Sums the event pairs of one stage over a pass."""
    def __init__(self):
        self.pairs = []

    def __call__(self, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self.pairs.append((e0, e1))
        return out

    def ms(self):
        torch.cuda.synchronize()
        t = sum(a.elapsed_time(b) for a, b in self.pairs)
        self.pairs = []
        return t


def med(xs):
    return statistics.median(xs), min(xs), max(xs)


def bench(D, reps):
    g = torch.Generator(device=dev).manual_seed(D)
    centres = torch.randn(64, D, device=dev, generator=g)
    bank = centres[torch.randint(0, 64, (N,), device=dev, generator=g)] + 0.9 * torch.randn(N, D, device=dev, generator=g)
    cohort = centres[torch.randint(0, 64, (M,), device=dev, generator=g)] + 0.9 * torch.randn(M, D, device=dev, generator=g)
    pairs = torch.randint(0, N, (P, 2), device=dev, generator=g, dtype=torch.int32)
    mean, std = ops.embed_stats(bank)
    ldS = (M + 3) // 4 * 4
    rpb = ops.cohort_rows_per_block(N, M)
    S = torch.empty(rpb, ldS, device=dev)
    u_buf, inv_buf = torch.empty(rpb, D, device=dev), torch.empty(rpb, device=dev)
    c_u, c_inv = torch.empty(M, D, device=dev), torch.empty(M, device=dev)
    mu, sd = torch.empty(N, device=dev), torch.empty(N, device=dev)
    cos, score, normed = torch.empty(P, device=dev), torch.empty(P, device=dev), torch.empty(P, device=dev)
    say(f"--- D = {D}: bank {N:,} x {D} ({N * D * 4 / 1e6:.0f} MB), cohort {M:,} x {D}, K = {K}, {P:,} trials; blocks of {rpb:,} "
        f"rows, workspace {rpb * ldS * 4 / 2 ** 20:.0f} MiB")
    t = {k: [] for k in ("transform", "product", "topk", "trials", "whole")}
    st = {k: Stage() for k in ("transform", "product", "topk", "trials", "whole")}
    kernel = None
    for rep in range(reps + 1):
        st["transform"](lambda: ops.rows_transform(cohort, mean, std, True, out=c_u, inv_norm=c_inv))
        for r0 in range(0, N, rpb):
            rows = min(rpb, N - r0)
            u, inv = st["transform"](lambda: ops.rows_transform(bank[r0:r0 + rows], mean, std, True, out=u_buf, inv_norm=inv_buf))
            gm = ops.Gemm(rows, M, D, u, c_u, S, lda=D, ldb=D, ldc=ldS, epilogue=ops.EPI_SCALE_RC, row_scale=inv, col_scale=c_inv)
            kernel = gm.kernel_name
            st["product"](gm)
            st["topk"](lambda: ops.topk_stats(S[:rows], K, M, mu[r0:r0 + rows], sd[r0:r0 + rows]))
        st["trials"](lambda: (ops.score_pairs(bank, pairs, mean, std, True, cos, score),
                              ops.score_pairs_norm(cos, pairs, mu, sd, "s", normed)))
        st["whole"](lambda: ops.cohort_stats(bank, cohort, K, mean, std, True, workspace=S))
        ms = {k: s.ms() for k, s in st.items()}
        if rep:                                            # (pass 0 is the warm-up)
            for k in t:
                t[k].append(ms[k])
    flops = 2.0 * N * M * D
    m_, lo, hi = med(t["transform"])
    nb = (N + M) * D * 4 * 2
    say(f"{'device transform (cohort + every block)':52s} median {m_:9.3f} ms  min {lo:9.3f}  max {hi:9.3f}   {nb / 1e6:8.0f} MB "
        f"read + written  {nb / m_ / 1e6:7.1f} GB/s")
    m_, lo, hi = med(t["product"])
    say(f"{'device product (' + kernel + ')':52s} median {m_:9.3f} ms  min {lo:9.3f}  max {hi:9.3f}   {flops / 1e12:.2f} TFLOP  "
        f"{flops / m_ / 1e9:6.1f} TFLOP/s = {100 * flops / m_ / 1e9 / F32_MATRIX_TFLOPS:.0f} % of the sustained f32 matrix rate "
        f"({F32_MATRIX_TFLOPS} TFLOP/s)")
    m_, lo, hi = med(t["topk"])
    nb = N * M * 4
    say(f"{'device topk_stats':52s} median {m_:9.3f} ms  min {lo:9.3f}  max {hi:9.3f}   S read once: {nb / 1e6:8.0f} MB  "
        f"{nb / m_ / 1e6:7.1f} GB/s (the product wrote the same bytes just before: L2 / HBM)")
    topk_ms = m_
    m_, lo, hi = med(t["trials"])
    say(f"{'device trial pass (score_pairs + score_pairs_norm)':52s} median {m_:9.3f} ms  min {lo:9.3f}  max {hi:9.3f}")
    m_, lo, hi = med(t["whole"])
    say(f"{'device ops.cohort_stats, whole':52s} median {m_:9.3f} ms  min {lo:9.3f}  max {hi:9.3f}")
    whole_ms = m_
    # the same computation in torch on the same device
    tt = {k: [] for k in ("transform", "product", "topk", "whole")}
    ts = {k: Stage() for k in tt}
    mu_t, sd_t = torch.empty(N, device=dev), torch.empty(N, device=dev)

    def transform(x):
        x = torch.nn.functional.normalize((x - mean) / (std + 1e-12), dim=1)
        return x / torch.linalg.vector_norm(x, dim=1, keepdim=True).clamp_min(1e-8)
    for rep in range(reps + 1):
        e = ts["whole"]
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        cn = ts["transform"](lambda: transform(cohort))
        for r0 in range(0, N, rpb):
            rows = min(rpb, N - r0)
            un = ts["transform"](lambda: transform(bank[r0:r0 + rows]))
            St = ts["product"](lambda: torch.matmul(un, cn.t()))

            def stats():
                top = torch.topk(St, K, dim=1).values
                mu_t[r0:r0 + rows] = top.mean(dim=1)
                sd_t[r0:r0 + rows] = top.std(dim=1)
            ts["topk"](stats)
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        e.pairs.append((e0, e1))
        ms = {k: s.ms() for k, s in ts.items()}
        if rep:
            for k in tt:
                tt[k].append(ms[k])
    for k, name in (("transform", "torch transform"), ("product", "torch matmul (f32)"), ("topk", "torch topk + mean + std"),
                    ("whole", "torch, whole")):
        m_, lo, hi = med(tt[k])
        extra = f"   {flops / m_ / 1e9:6.1f} TFLOP/s" if k == "product" else ""
        say(f"{name:52s} median {m_:9.3f} ms  min {lo:9.3f}  max {hi:9.3f}{extra}")
    d_mu, d_sd = (mu - mu_t).abs().max().item(), (sd - sd_t).abs().max().item()
    say(f"device vs torch on these inputs: |mu difference| {d_mu:.2e}, |sd difference| {d_sd:.2e}; torch whole / device whole = "
        f"{statistics.median(tt['whole']) / whole_ms:.2f}; topk_stats is {100 * topk_ms / whole_ms:.0f} % of the device pass")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="+", default=[192, 1536])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "score_norm_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the GPU: no device, no numbers"
    say(f"tools/score_norm_bench.py --reps {a.reps}: {torch.cuda.get_device_name(0)}; HIP events, one warm-up pass, median / min / "
        f"max of {a.reps} passes")
    for D in a.dims:
        bench(D, a.reps)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
