"""Time the margin heads (heads.ClassifierHead with sub-centres / inter-top-k) at the training shape, next to the default
single-centre head and to the same head written in eager torch on the device -> profiles/margin_head_bench.txt.

B = 66, C = 5994, E in {192, 1536}, K in {1, 3}, inter_topk in {0, 5}, f32 and bf16.  Per case, in ONE process: the
head under test, the default head (K = 1, w2v2_aam_softmax_fwd_bwd) and the eager-torch twin (F.normalize, matmul in the
operand dtype, view(B, C, K).max, topk, where, cross_entropy, autograd), each ``forward_backward`` timed with HIP events:
50 timed calls after 10 warm-up calls, median / p10 / p90 in microseconds.  The row kernel alone is timed the same way,
so the cost of the selection rounds stands next to the kernel without them.  The K = 1, inter_topk = 0 line runs the
NEW entry on the default problem (the head is told to; the default path never calls it) next to the old kernel's time.

What a non-default form has to meet: no slower than its eager-torch twin (the last column says so).

    python tools/margin_head_bench.py [--out profiles/margin_head_bench.txt]

The parent starts one child process per case, one at a time, each under its own time limit, and stops at the first that
fails; it never touches the GPU itself."""
import argparse
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, C = 66, 5994
MARGIN, SCALE, INTER_MARGIN = 0.2, 30.0, 0.06
WARMUP, REPS = 10, 50
CASE_TIMEOUT = 240
CASES = [(E, K, top, dt) for E in (192, 1536) for dt in ("f32", "bf16") for K in (1, 3) for top in (0, 5)]


def timed(fn):
    """-> (median, p10, p90) in microseconds of REPS calls, each between its own pair of HIP events."""
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[REPS // 2], t[REPS // 10], t[REPS - 1 - REPS // 10]


def fmt(t):
    return f"median {t[0]:8.1f} us  p10 {t[1]:8.1f}  p90 {t[2]:8.1f}"


def run_case(E: int, K: int, top: int, dts: str) -> None:
    import torch
    import torch.nn.functional as F
    from w2v2_speaker_amd import ops
    from w2v2_speaker_amd.heads import ClassifierHead
    dev, dtype = "cuda", {"f32": torch.float32, "bf16": torch.bfloat16}[dts]
    g = torch.Generator().manual_seed(E + K)
    W = (torch.randn(C * K, E, generator=g) * math.sqrt(2.0 / (C * K + E))).to(dev)
    emb = torch.randn(B, E, generator=g).to(dev)
    label = torch.randint(0, C, (B,), generator=g).to(dev)

    def make(k, n_top, force_new=False):
        wm = W[:C * k].contiguous()
        wlp = wm if dtype == torch.float32 else wm.to(dtype)
        head = ClassifierHead("aam", B, E, C, w_master=wm, w_operand=wlp, w_grad=torch.zeros_like(wm), emb=emb.clone(),
                              act_dtype=dtype, train=True, margin=MARGIN, scale=SCALE, sub_centers=k, inter_topk=n_top,
                              inter_margin=INTER_MARGIN)
        if force_new:
            head.margin_head = True
        return head

    def eager():
        x, w = emb.detach().requires_grad_(True), W.detach().requires_grad_(True)
        cos = (F.normalize(x).to(dtype) @ F.normalize(w).to(dtype).t()).float()
        m = cos.view(B, C, K).max(dim=2).values
        one_hot = torch.zeros_like(m, dtype=torch.bool).scatter_(1, label.view(-1, 1), True)
        sine = torch.sqrt((1.0 - m * m).clamp(0, 1))
        phi = m * math.cos(MARGIN) - sine * math.sin(MARGIN)
        phi = torch.where(m - math.cos(math.pi - MARGIN) > 0, phi, m - math.sin(math.pi - MARGIN) * MARGIN)
        z = m
        if top:
            idx = m.detach().masked_fill(one_hot, float("-inf")).topk(top, dim=1).indices
            sel = torch.zeros_like(one_hot).scatter_(1, idx, True)
            z = torch.where(sel, m * math.cos(INTER_MARGIN) + sine * math.sin(INTER_MARGIN), m)
        loss = F.cross_entropy(torch.where(one_hot, phi, z) * SCALE, label)
        loss.backward()
        return loss

    new = make(K, top, force_new=(K, top) == (1, 0))
    old = make(1, 0)
    assert new.margin_head and not old.margin_head
    la, lb = float(new.forward_backward(label)[0]), float(eager())
    assert abs(la - lb) < (1e-4 if dtype == torch.float32 else 3e-2) * abs(lb), (la, lb)
    t_new, t_old, t_eager = timed(lambda: new.forward_backward(label)), timed(lambda: old.forward_backward(label)), timed(eager)

    def row(head):
        if head.margin_head:
            return lambda: ops.margin_softmax_fwd_bwd(
                head.logits, label, head.softmax, head.loss_rows, head.dcos_w, head.dcos_x, head.inv_x, head.inv_w,
                head.rowdot, head.colprod, B, C, head.K, head.ldc, head.ldp, MARGIN, SCALE, None, head.correct,
                n_top=head.inter_topk, inter_margin=INTER_MARGIN)
        return lambda: ops.aam_softmax_fwd_bwd(head.logits, label, head.softmax, head.loss_rows, head.dcos_w, head.dcos_x,
                                               head.inv_x, head.inv_w, head.rowdot, head.colprod, B, C, head.ldc, MARGIN,
                                               SCALE, None, head.correct)

    r_new, r_old = timed(row(new)), timed(row(old))
    r_sel = ""
    if top:
        r_sel = f"; the same kernel without the {top} selection rounds {timed(row(make(K, 0, force_new=True)))[0]:.1f} us"
    verdict = "(no gate: the default path does not call the new entry)" if (K, top) == (1, 0) else \
        ("no slower than eager torch: yes" if t_new[0] <= t_eager[0] else "no slower than eager torch: NO")
    tag = f"E={E:4d} K={K} inter_topk={top} {dts:4s}"
    print(f"{tag}  head, margin entry   {fmt(t_new)}   loss {la:.5f}")
    print(f"{tag}  head, default (K=1)  {fmt(t_old)}")
    print(f"{tag}  eager torch twin     {fmt(t_eager)}   loss {lb:.5f}   eager / head = {t_eager[0] / t_new[0]:.2f}  {verdict}")
    print(f"{tag}  row kernel alone     {fmt(r_new)}   aam_row_kernel (K=1) {r_old[0]:.1f} us{r_sel}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "margin_head_bench.txt"))
    ap.add_argument("--case", default=None, help="E,K,inter_topk,dtype: run this one case in this process")
    a = ap.parse_args()
    if a.case:
        E, K, top, dts = a.case.split(",")
        run_case(int(E), int(K), int(top), dts)
        return 0
    lines = [f"tools/margin_head_bench.py: ClassifierHead.forward_backward at B = {B}, C = {C}, margin {MARGIN}, scale "
             f"{SCALE:g}, inter_margin {INTER_MARGIN}; HIP events around each call, {WARMUP} warm-up + {REPS} timed calls, "
             "one process per case"]
    rc = 0
    for E, K, top, dts in CASES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", f"{E},{K},{top},{dts}"],
                               capture_output=True, text=True, timeout=CASE_TIMEOUT)
        except subprocess.TimeoutExpired:
            lines.append(f"E={E} K={K} inter_topk={top} {dts}: no result within {CASE_TIMEOUT} s; stopped here")
            rc = 124
            break
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("E=")]
        print("\n".join(r.stdout.splitlines()), flush=True)
        if r.returncode != 0:
            lines.append(f"E={E} K={K} inter_topk={top} {dts}: exit status {r.returncode}; stopped here")
            print(r.stderr[-2000:], file=sys.stderr)
            rc = r.returncode
            break
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
