"""Timing of the LDA / PLDA scoring back-ends (csrc/backend.hip + the exact-f32 GEMM + the float64 host solves) at the size
of a VoxCeleb2 fit and a VoxCeleb1-E evaluation:
  fit      a 200,000 x 1,536 training bank of 5,994 speakers, R = 200, Q = 150, 10 EM steps, by part: class means and
           global mean, the two scatter passes (centring, f32 block products against the sustained f32 matrix rate, the
           float64 fold), the host solves (two [D, D] copies + the eigen-solves), the latent pass (projection, statistics,
           transform, the latent scatter) and the EM + diagonalisation
  scoring  579,818 trials over a 145,160-row bank: projection, latent transform, diagonalising projection, llr kernel
each beside the same computation in torch on the same device and in float64 numpy on the host.  HIP events around device
work, a host clock around work that ends in a synchronise; one warm-up pass, then the median of --reps passes.  No time
target is asserted; the file records what came out.
    python tools/backend_bench.py [--reps 3] [--out profiles/backend_bench.txt]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from w2v2_speaker_amd import ops
from w2v2_speaker_amd.evaluation.speaker import PLDAEvaluator, backend
from w2v2_speaker_amd.evaluation.speaker.device_scoring import TrialIndex, _upload

dev = "cuda"
F32_MATRIX_TFLOPS = 153.7      # profiles/r05_mfma_f32_sustained.txt (tools/probes/mfma_f32_sustained_probe.hip)
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn):
    """(result, ms) of device work by a pair of HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def wall(fn):
    """(result, ms) by the host clock around work that ends in a synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def line(name, xs, extra=""):
    say(f"{name:58s} median {statistics.median(xs):10.3f} ms  min {min(xs):10.3f}  max {max(xs):10.3f}{extra}")


def scatter_by_part(bank, seg, means, weight, rpb, acc_ms, blocks_per_launch):
    """ops.class_scatter's own block loop (``blocks_per_launch`` block products per batched GEMM launch) with an event pair
    around each stage."""
    N, D = bank.shape
    rpb = min(rpb, N)
    G = max(1, min(blocks_per_launch, N // rpb))
    a_buf, prod = torch.empty(G * rpb, D, device=dev), torch.empty(G, D, D, device=dev)
    acc = torch.empty(D, D, dtype=torch.float64, device=dev)
    name, r0 = None, 0
    while r0 < N:
        g = min(G, (N - r0) // rpb)
        k = rpb if g else N - r0
        g = max(g, 1)
        rows = g * k
        _, ms = timed(lambda: ops.rows_center(bank[r0:r0 + rows], means, None if seg is None else seg[r0:r0 + rows],
                                              None if weight is None else weight[r0:r0 + rows], out=a_buf))
        acc_ms["centre"] += ms
        gm = ops.Gemm(D, D, k, a_buf, a_buf, prod, lda=D, ldb=D, ldc=D, transA=True, transB=True, batch=g,
                      a_strides=(k * D, 0), b_strides=(k * D, 0), c_strides=(D * D, 0))
        name = gm.kernel_name
        _, ms = timed(gm)
        acc_ms["product"] += ms
        _, ms = timed(lambda: [ops.scatter_fold(prod[z], acc, first=r0 == 0 and z == 0) for z in range(g)])
        acc_ms["fold"] += ms
        r0 += rows
    return acc, name


def bench_fit(a):
    N, D, C, R, Q, its = a.rows, a.dim, a.speakers, a.components, a.plda_components, a.iterations
    g = torch.Generator(device=dev).manual_seed(1)
    ids = np.sort(np.concatenate([np.arange(C), np.random.default_rng(1).integers(0, C, N - C)]))
    ids_d = _upload(ids.astype(np.int32), dev)
    scale = torch.linspace(1.0, 0.05, D, device=dev)
    bank = (torch.randn(C, D, device=dev, generator=g) * scale)[ids_d.long()] + torch.randn(N, D, device=dev, generator=g) * 0.7 + 0.5
    order, offsets, counts = backend.segments(ids, C)
    order_d, offsets_d = _upload(order, dev), _upload(offsets, dev)
    root_n = _upload(np.sqrt(counts).astype(np.float32), dev)
    say(f"--- fit: bank {N:,} x {D} ({N * D * 4 / 1e6:.0f} MB), {C:,} speakers ({len(np.unique(counts))} distinct counts), R = {R}, "
        f"Q = {Q}, {its} EM steps, scatter blocks of {ops.SCATTER_ROWS_PER_BLOCK} rows")
    t = {k: [] for k in ("means", "centre", "product", "fold", "sb", "copy", "solve", "whole", "product1")}
    kernel = None
    for rep in range(a.reps + 1):
        (means, mu0), ms_means = timed(lambda: (ops.segment_mean(bank, order_d, offsets_d), ops.embed_stats(bank)[0]))
        part = {"centre": 0.0, "product": 0.0, "fold": 0.0}
        Sw, kernel = scatter_by_part(bank, ids_d, means, None, ops.SCATTER_ROWS_PER_BLOCK, part, ops.SCATTER_BLOCKS_PER_LAUNCH)
        one = {"centre": 0.0, "product": 0.0, "fold": 0.0}
        scatter_by_part(bank, ids_d, means, None, ops.SCATTER_ROWS_PER_BLOCK, one, 1)
        Sb, ms_sb = timed(lambda: ops.class_scatter(means, None, mu0.view(1, D), row_weight=root_n))
        (Sw_h, Sb_h), ms_copy = wall(lambda: (Sw.cpu(), Sb.cpu()))
        stats = backend.ClassStatistics(torch.from_numpy(counts.astype(np.float64)), means.cpu().double(), mu0.cpu().double(),
                                        backend._sym(Sw_h), backend._sym(Sb_h))
        _, ms_solve = wall(lambda: backend.solve_projection(stats, R, "pca"))
        ev = PLDAEvaluator(R, Q, its, 0)
        _, ms_whole = wall(lambda: ev.fit_parameters_bank(bank, ids))
        if rep:
            for k, v in (("means", ms_means), ("sb", ms_sb), ("copy", ms_copy), ("solve", ms_solve), ("whole", ms_whole)):
                t[k].append(v)
            for k in part:
                t[k].append(part[k])
            t["product1"].append(one["product"])
    flops = 2.0 * N * D * D
    line("device class means + global mean", t["means"], f"   {N * D * 4 * 2 / 1e6:.0f} MB read")
    line("device S_w: rows_center", t["centre"], f"   {N * D * 8 / statistics.median(t['centre']) / 1e6:7.1f} GB/s read + written")
    m_ = statistics.median(t["product"])
    line(f"device S_w: A^T A ({kernel})", t["product"], f"   {flops / 1e12:.2f} TFLOP  {flops / m_ / 1e9:6.1f} TFLOP/s = "
         f"{100 * flops / m_ / 1e9 / F32_MATRIX_TFLOPS:.0f} % of the sustained f32 matrix rate ({F32_MATRIX_TFLOPS} TFLOP/s)")
    m1 = statistics.median(t["product1"])
    line("   ... with one block product per launch", t["product1"], f"   {flops / m1 / 1e9:6.1f} TFLOP/s = "
         f"{100 * flops / m1 / 1e9 / F32_MATRIX_TFLOPS:.0f} % ({ops.SCATTER_BLOCKS_PER_LAUNCH} per launch is ops.class_scatter's)")
    nblk = -(-N // ops.SCATTER_ROWS_PER_BLOCK)
    line("device S_w: scatter_fold", t["fold"], f"   {nblk} blocks x {D * D * 20 / 1e6:.0f} MB")
    line("device S_b (class_scatter over the class means)", t["sb"])
    line("two [D, D] float64 matrices to the host", t["copy"])
    line("host projection solve (float64 eigh)", t["solve"])
    line("fit_parameters_bank, whole (PLDA: + latent pass, EM)", t["whole"])
    # the latent pass and the EM, once more by part on the fitted evaluator's own data
    tl = {k: [] for k in ("latent", "em")}
    for rep in range(a.reps + 1):
        def latent():
            Y = ev._project(bank)
            mean, std = ops.embed_stats(Y)
            Z, _ = ops.rows_transform(Y, mean, std, True)
            zm = ops.segment_mean(Z, order_d, offsets_d)
            return zm, ops.embed_stats(Z)[0], ops.class_scatter(Z, ids_d, zm)
        (zm, zmu, zSw), ms_lat = timed(latent)
        zm_h, zmu_h, zSw_h = zm.cpu().double()[:, :R], zmu.cpu().double()[:R], backend._sym(zSw.cpu())[:R, :R]
        t0 = time.perf_counter()
        backend.solve_plda(torch.from_numpy(counts.astype(np.float64)), zm_h, zmu_h, zSw_h, Q, its)
        ms_em = (time.perf_counter() - t0) * 1e3
        if rep:
            tl["latent"].append(ms_lat)
            tl["em"].append(ms_em)
    line("device latent pass (project, stats, transform, S_w of Z)", tl["latent"])
    line(f"host EM ({its} steps) + diagonalisation (float64)", tl["em"])
    # the same statistics in torch on the same device (f32 matmul, f32 sums)
    tt = []
    for rep in range(a.reps + 1):
        def torch_stats():
            idl = ids_d.long()
            m = torch.zeros(C, D, device=dev).index_add_(0, idl, bank) / torch.bincount(idl, minlength=C)[:, None]
            Xc = bank - m[idl]
            Mc = (m - bank.mean(dim=0)) * torch.bincount(idl, minlength=C).sqrt()[:, None]
            return Xc.t() @ Xc, Mc.t() @ Mc
        (Sw_t, Sb_t), ms = timed(torch_stats)
        if rep:
            tt.append(ms)
    line("torch on the device: means + S_w + S_b (f32 matmul)", tt)
    dev_stats = statistics.median(t["means"]) + statistics.median(t["centre"]) + statistics.median(t["product"]) + \
        statistics.median(t["fold"]) + statistics.median(t["sb"])
    rel = lambda A, B: float((A - B).abs().max() / B.abs().max())
    # float64 numpy on the host
    t0 = time.perf_counter()
    X = bank.cpu().numpy().astype(np.float64)
    cnt = np.bincount(ids, minlength=C)
    m64 = np.add.reduceat(X[order], offsets[:-1], axis=0) / cnt[:, None]
    Xc = X - m64[ids]
    Sw64 = Xc.T @ Xc
    Mc = (m64 - X.mean(axis=0)) * np.sqrt(cnt)[:, None]
    Sb64 = Mc.T @ Mc
    ms_np = (time.perf_counter() - t0) * 1e3
    say(f"{'float64 numpy on the host: means + S_w + S_b (one pass)':58s}        {ms_np:10.3f} ms")
    Sw64_t, Sb64_t = torch.from_numpy(Sw64), torch.from_numpy(Sb64)
    say(f"device statistics {dev_stats:.3f} ms against torch {statistics.median(tt):.3f} ms and numpy float64 {ms_np:.0f} ms; "
        f"max |S_w - float64| / max |S_w|: device {rel(backend._sym(Sw_h), backend._sym(Sw64_t)):.2e}, torch f32 "
        f"{rel(backend._sym(Sw_t.cpu().double()), backend._sym(Sw64_t)):.2e}; S_b: device "
        f"{rel(backend._sym(Sb_h), backend._sym(Sb64_t)):.2e}, torch f32 {rel(backend._sym(Sb_t.cpu().double()), backend._sym(Sb64_t)):.2e}")
    say()
    return ev


def bench_scoring(a, ev):
    N, D, P = a.bank_rows, a.dim, a.trials
    g = torch.Generator(device=dev).manual_seed(2)
    scale = torch.linspace(1.0, 0.05, D, device=dev)
    bank = (torch.randn(1251, D, device=dev, generator=g) * scale)[torch.randint(0, 1251, (N,), device=dev, generator=g)] \
        + torch.randn(N, D, device=dev, generator=g) * 0.7 + 0.5
    rows = np.random.default_rng(3).integers(0, N, (P, 2))
    index = TrialIndex.from_rows(rows, np.random.default_rng(4).integers(0, 2, P), N)
    table = index.device_table(dev)
    m = ev._device_model(dev)
    say(f"--- scoring: bank {N:,} x {D}, {P:,} trials, R = {a.components}, Q = {a.plda_components}")
    t = {k: [] for k in ("project", "transform", "diag", "llr", "whole")}
    for rep in range(a.reps + 1):
        Y, ms_p = timed(lambda: ev._project(bank))
        (Z, _), ms_t = timed(lambda: ops.rows_transform(Y, m["mean"], m["std"], True))
        U, ms_d = timed(lambda: ev._project(Z, "diag_"))
        llr, ms_l = timed(lambda: ops.plda_score_pairs(U, table, m["p"], m["q"], ev._k))
        rec, ms_w = wall(lambda: ev._device_scores(bank, index, True, None))
        if rep:
            for k, v in (("project", ms_p), ("transform", ms_t), ("diag", ms_d), ("llr", ms_l), ("whole", ms_w)):
                t[k].append(v)
    flops = 2.0 * N * D * Y.shape[1]
    line("device projection (f32 GEMM + bias)", t["project"], f"   {flops / statistics.median(t['project']) / 1e9:6.1f} TFLOP/s")
    line("device latent transform (rows_transform)", t["transform"])
    line("device diagonalising projection (f32 GEMM + bias)", t["diag"])
    nb = P * 2 * U.shape[1] * 4
    line("device plda_score_pairs", t["llr"], f"   {nb / 1e6:.0f} MB of rows gathered  {nb / statistics.median(t['llr']) / 1e6:7.1f} GB/s")
    line("device scoring, whole (scores left on the device)", t["whole"])
    tt = []
    p32, q32 = m["p"].float(), m["q"].float()
    for rep in range(a.reps + 1):
        def torch_score():
            y = torch.nn.functional.normalize((bank @ m["w"].t() + m["b"] - m["mean"]) / (m["std"] + 1e-12), dim=1)
            u = y @ m["diag_w"].t() + m["diag_b"]
            ue, ut = u[table[:, 0].long()], u[table[:, 1].long()]
            return ev._k + (ue * ut * p32).sum(dim=1) - ((ue * ue + ut * ut) * q32).sum(dim=1)
        llr_t, ms = timed(torch_score)
        if rep:
            tt.append(ms)
    line("torch on the device: the same chain (f32)", tt)
    t0 = time.perf_counter()
    X = bank.cpu().numpy().astype(np.float64)
    w, b = ev._proj_w.double().numpy(), ev._proj_b.double().numpy()
    y = (X @ w.T + b - ev._mean.double().numpy()) / (ev._std.double().numpy() + 1e-12)
    y /= np.maximum(np.linalg.norm(y, axis=1, keepdims=True), 1e-12)
    u = y @ ev._diag_w.double().numpy().T + ev._diag_b.double().numpy()
    ue, ut = u[rows[:, 0]], u[rows[:, 1]]
    p, q = ev._p.numpy(), ev._q.numpy()
    llr64 = ev._k + (ue * ut * p).sum(axis=1) - ((ue * ue + ut * ut) * q).sum(axis=1)
    ms_np = (time.perf_counter() - t0) * 1e3
    say(f"{'float64 numpy on the host: the same chain':58s}        {ms_np:10.3f} ms")
    d_dev = np.abs(rec.device_scores.cpu().numpy() - llr64).max()
    d_t = np.abs(llr_t.cpu().numpy() - llr64).max()
    say(f"max |llr - float64| with the same fitted model: device {d_dev:.2e}, torch f32 {d_t:.2e}, at |llr| max {np.abs(llr64).max():.2e}; "
        f"torch / device = {statistics.median(tt) / statistics.median(t['whole']):.2f}")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--speakers", type=int, default=5994)
    ap.add_argument("--components", type=int, default=200)
    ap.add_argument("--plda-components", type=int, default=150)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--bank-rows", type=int, default=145160)
    ap.add_argument("--trials", type=int, default=579818)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "backend_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the GPU: no device, no numbers"
    say(f"tools/backend_bench.py --reps {a.reps}: {torch.cuda.get_device_name(0)}; HIP events around device work, a host clock "
        f"around host work, one warm-up pass, median / min / max of {a.reps} passes")
    ev = bench_fit(a)
    bench_scoring(a, ev)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
