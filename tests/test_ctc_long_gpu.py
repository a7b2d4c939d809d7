"""GPU tests of the long-target CTC loss (w2v2_ctc_long_fwd_bwd, csrc/ctc_long.hip) against the float64 reference of
tests/ctc_long_cases.py, of the greedy decoder (w2v2_ctc_greedy_decode) against the Python loop it replaces, and of
``CtcLoss(long_targets=True)``.

Bounds (tests/ctc_cases.py): loss rows 2e-5 relative to max(1, |ref|); gradient rel-L2 per utterance, the largest over the
batch, at most max(1e-5, 2 x the error of torch's own f32 CPU F.ctc_loss on the same inputs).  tests/test_ctc_long_cpu.py
shows that the kernel's arithmetic restated in f32 on the CPU meets them, so a miss here is the kernel's.  Lines that
start with ``ctc-long-parity:`` are the measured figures recorded in profiles/ctc_long_parity.txt."""
import pytest
import torch

import ctc_cases as CC
import ctc_long_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
SENT = -7.0


def ops():
    from w2v2_speaker_amd import ops as o
    return o


def say(what, figures):
    print("ctc-long-parity: " + what + ": " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}"
                                                          for k, v in figures.items()))


def device_logits(c):
    """[B*T, ldc] f32 on the device, NaN in the padding columns."""
    B, T, C = c["logits"].shape
    z = torch.full((B * T, c["ldc"]), float("nan"), dtype=F32)
    z[:, :C] = c["logits"].reshape(B * T, C)
    return z.to(DEV)


def launch(c, *, grad=F32, loss_scale=None, targets=None, tgt_len=None, in_len=None, offset=0, short=False, keep_ws=False):
    """One launch into sentinel-filled outputs and a NaN-filled workspace -> (loss_rows [B], dlogits [B, T, ldc] or None
    [, workspace]), device tensors.  ``short``: the entry of csrc/ctc.hip instead."""
    o = ops()
    B, T, C = c["logits"].shape
    ldc = c["ldc"]
    z = device_logits(c)
    tg = (c["targets"] if targets is None else targets).to(DEV)
    il = (c["in_len"] if in_len is None else in_len).to(DEV)
    tl = (c["tgt_len"] if tgt_len is None else tgt_len).to(DEV)
    rows = torch.full((B,), SENT, dtype=F32, device=DEV)
    dl = None if grad is None else torch.full((B * T, ldc), SENT, dtype=grad, device=DEV)
    floats, fn = (o.ctc_workspace_floats, o.ctc_fwd_bwd) if short else (o.ctc_long_workspace_floats, o.ctc_long_fwd_bwd)
    ws = torch.full((floats(B, T, tg.shape[1]),), float("nan"), dtype=F32, device=DEV)
    ls = None if loss_scale is None else torch.tensor([loss_scale, 0.0, 0.0, 0.0], device=DEV)
    fn(z, tg, il, tl, rows, dl, ws, B, T, C, ldc, target_width=tg.shape[1], target_offset=offset, blank=c["blank"],
       loss_scale=ls)
    torch.cuda.synchronize()
    out = (rows, None if dl is None else dl.view(B, T, ldc))
    return out + (ws,) if keep_ws else out


@pytest.mark.parametrize("name", LC.CASES)
def test_kernel_against_float64(name):
    c = LC.case(name)
    C = c["logits"].shape[2]
    rows, dl = launch(c)
    assert bool((dl[..., C:] == SENT).all()), "the padding columns are not the kernel's to write"
    e = LC.errors(c, rows, dl[..., :C])
    say(name, {**e, "bound": LC.grad_bound(name), "torch_f32": LC.ref_f32_error(name)})
    assert e["loss_rows"] < LC.LOSS_TOL
    assert e["grad"] <= LC.grad_bound(name)
    assert e["zeros_ok"], "infeasible utterances and frames past an utterance's end get exact zeros"
    assert e["row_sum"] < 2e-5          # (the bound of tests/test_ctc_gpu.py: softmax and posteriors both sum to one)
    for b in c["infinite"]:
        assert float(rows[b]) == 0.0


@pytest.mark.parametrize("name", CC.SMALL_CASES)
def test_both_entries_meet_the_bounds_at_short_widths(name):
    c = CC.case(name)
    C = c["logits"].shape[2]
    for short in (True, False):
        rows, dl = launch(c, short=short)
        e = CC.errors(c, rows, dl[..., :C])
        say(f"{name} ({'short' if short else 'long'} entry)", {**e, "bound": CC.grad_bound(name)})
        assert e["loss_rows"] < CC.LOSS_TOL and e["grad"] <= CC.grad_bound(name) and e["zeros_ok"]
        assert bool((dl[..., C:] == SENT).all())


def test_two_launches_are_bitwise_equal():
    for name in ("mixed_long", "pairs", "c29_nan_padding", "c5995_wide"):
        c = LC.case(name)
        C = c["logits"].shape[2]
        r1, d1 = launch(c)
        r2, d2 = launch(c)
        assert torch.equal(r1, r2) and torch.equal(d1[..., :C], d2[..., :C]), name


def test_forward_only_and_loss_scale_and_offset():
    c = LC.case("w33")
    C = c["logits"].shape[2]
    r1, d1 = launch(c)
    rows, none = launch(c, grad=None)
    assert none is None and torch.equal(rows, r1)
    r2, d2 = launch(c, loss_scale=1024.0)
    assert torch.equal(r1, r2) and torch.equal(d2[..., :C], d1[..., :C] * 1024.0)        # a power of two: exact
    r3, d3 = launch(c, targets=c["targets"] - 1, offset=1)
    assert torch.equal(r1, r3) and torch.equal(d1[..., :C], d3[..., :C])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16_bit_gradient_is_the_f32_one_rounded(dtype):
    for name, scale in (("l257", 256.0), ("c29_nan_padding", 1.0), ("c5995_wide", 1.0)):
        c = LC.case(name)
        C = c["logits"].shape[2]
        _, d32 = launch(c, loss_scale=scale)
        _, d16 = launch(c, grad=dtype, loss_scale=scale)
        assert torch.equal(d16[..., :C], d32[..., :C].to(dtype))
        assert bool((d16[..., C:] == SENT).all())


def test_bad_rows_are_nan_with_zero_gradients():
    """A label equal to the blank, a class >= C, a target length above the width, an input length above T: NaN loss row,
    zero gradient, the good rows as before (nothing out of range is read: the bad classes point far outside the logits),
    and the bad row's part of the workspace -- row statistics, emissions, lattice -- stays as the test filled it."""
    o = ops()
    c = LC.case("wide_bias100")
    B, T, C = c["logits"].shape
    W = c["targets"].shape[1]
    good_rows, good = launch(c)
    for what in ("class_high", "class_negative", "blank", "target_length", "input_length"):
        tg, tl, il = c["targets"].clone(), c["tgt_len"].clone(), c["in_len"].clone()
        if what == "class_high":
            tg[0, 37] = C + (1 << 40)
        elif what == "class_negative":
            tg[0, 0] = -(1 << 40)
        elif what == "blank":
            tg[0, 33] = c["blank"]
        elif what == "target_length":
            tl[0] = W + 1
        else:
            il[0] = T + 1
        rows, dl, ws = launch(c, targets=tg, tgt_len=tl, in_len=il, keep_ws=True)
        assert bool(torch.isnan(rows[0])), what
        assert bool((dl[0, :, :C] == 0).all()), what
        assert bool((dl[..., C:] == SENT).all()), what
        keep = [1, 2, 3]
        assert torch.equal(rows[keep], good_rows[keep]) and torch.equal(dl[keep][..., :C], good[keep][..., :C]), what
        # the workspace: {status}[B] | row statistics [B*T] x 4 | chains | emissions 2 x [B*T][W + 1] | lattice [B*T][W + 1] x 4
        assert ws.numel() == o.ctc_long_workspace_floats(B, T, W)
        stat = ws[4 * B:4 * B + 4 * B * T].view(B, T, 4)
        assert bool(torch.isnan(stat[0]).all()) and bool(torch.isfinite(stat[1, :, :3]).all()), what
        lattice = ws[ws.numel() - 4 * B * T * (W + 1):].view(B, T, W + 1, 4)
        assert bool(torch.isnan(lattice[0]).all()), what
        assert not bool(torch.isnan(lattice[1][..., 0::2]).any()), what      # (1 and 3 are exponents: int bits)
    # a bad class beyond a row's target length is padding, not an error
    tg = c["targets"].clone()
    tg[1, 20] = -5
    rows, dl = launch(c, targets=tg)
    assert torch.equal(rows, good_rows) and torch.equal(dl[..., :C], good[..., :C])


def test_width_limit_is_a_host_error():
    c = LC.case("w32")
    with pytest.raises(ValueError):
        launch(c, targets=torch.ones(2, 1024, dtype=torch.int64))
    with pytest.raises(ValueError):
        launch(c, short=True)                      # the short entry still refuses 32 labels


def test_ctc_loss_module_with_long_targets():
    from w2v2_speaker_amd.optim.loss import CtcLoss
    c = LC.case("w33")
    ref = c["ref"]
    flat = torch.cat([c["targets"][b, :int(L)] for b, L in enumerate(c["tgt_len"])])
    for layout, targets in (("2d", c["targets"]), ("1d", flat)):
        x = c["logits"].to(DEV).requires_grad_(True)
        loss = CtcLoss(long_targets=True)(x, c["in_len"].to(DEV), targets.to(DEV), c["tgt_len"].to(DEV))
        (loss * 3.0).backward()
        fig = {"loss": abs(float(loss) - float(ref["loss"])) / max(1.0, float(ref["loss"])),
               "grad": CC.per_utterance_rel_l2(x.grad / 3.0, ref["grad"]), "bound": LC.grad_bound("w33")}
        say(f"CtcLoss long {layout}", fig)
        assert fig["loss"] < LC.LOSS_TOL and fig["grad"] <= LC.grad_bound("w33")
    # at a short width the long-target module runs the short kernels: bit for bit the default module's result
    s = CC.case("mixed")
    a = s["logits"].to(DEV).requires_grad_(True)
    b = s["logits"].to(DEV).requires_grad_(True)
    args = (s["in_len"].to(DEV), s["targets"].to(DEV), s["tgt_len"].to(DEV))
    la, lb = CtcLoss()(a, *args), CtcLoss(long_targets=True)(b, *args)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    with pytest.raises(ValueError, match="at most 31"):
        CtcLoss()(x, c["in_len"], c["targets"], c["tgt_len"])


# ------------------------------------------------------------------------------------------------------ greedy decoder
def python_decode(logits, in_len, blank):
    """ref: speech_recognition_module.py:233-248 without the tokenizer: argmax, collapse runs, drop the blank."""
    out = []
    for b in range(logits.shape[0]):
        idx = torch.argmax(logits[b, :int(in_len[b])], dim=1).tolist()
        seq, prev = [], None
        for i in idx:
            if i != prev and i != blank:
                seq.append(i)
            prev = i
        out.append(seq)
    return out


def device_decode(logits, in_len, blank, ldc=None):
    o = ops()
    B, T, C = logits.shape
    ldc = ldc or C
    z = torch.full((B * T, ldc), float("nan"), dtype=F32)
    z[:, :C] = logits.reshape(B * T, C)
    tokens = torch.full((B, T), -9, dtype=torch.int32, device=DEV)
    counts = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    o.ctc_greedy_decode(z.to(DEV), in_len.to(DEV), tokens, counts, B, T, C, ldc, blank=blank)
    tokens, counts = tokens.cpu(), counts.cpu()          # (one copy each; the default stream orders them)
    seqs = [tokens[b, :int(counts[b])].tolist() for b in range(B)]
    for b in range(B):
        assert bool((tokens[b, int(counts[b]):] == -9).all()), "entries past the count are not the kernel's to write"
    return seqs


def from_indices(rows, C, g):
    """Logits whose per-frame argmax is the given index (the winner 1 above noise in [0, 0.5))."""
    idx = torch.tensor(rows)
    z = torch.rand(idx.shape[0], idx.shape[1], C, generator=g) * 0.5
    z.scatter_(2, idx[..., None], 1.5)
    return z


def test_greedy_decoder_against_the_python_loop():
    g = torch.Generator().manual_seed(24)
    a, _ = 5, 0
    # `a a _ a` -> `a a`; all blank; a run across the whole row; T = 1
    z = from_indices([[a, a, _, a], [_, _, _, _], [a, a, a, a], [_, a, 7, 7]], 32, g)
    il = torch.tensor([4, 4, 4, 4], dtype=torch.int32)
    assert device_decode(z, il, 0) == python_decode(z, il, 0) == [[a, a], [], [a], [a, 7]]
    z1 = from_indices([[a], [_]], 32, g)
    il1 = torch.tensor([1, 1], dtype=torch.int32)
    assert device_decode(z1, il1, 0) == python_decode(z1, il1, 0) == [[a], []]
    # ties: the lowest index wins, as torch.argmax does (a row of equal values decodes to index 0 = blank)
    zt = torch.zeros(2, 6, 32)
    zt[0, :, 9] = zt[0, :, 4] = 2.0
    zt[1, 2, 31] = zt[1, 2, 30] = 1.0
    ilt = torch.tensor([6, 6], dtype=torch.int32)
    assert device_decode(zt, ilt, 0) == python_decode(zt, ilt, 0) == [[4], [30]]
    # chunk and wave edges of the frame loop, input lengths 0 and T, random sequences with many repeats
    for T in (63, 64, 65, 255, 256, 257, 600):
        idx = torch.randint(0, 4, (4, T), generator=g).tolist()
        z = from_indices(idx, 32, g)
        il = torch.tensor([T, 0, T - 1, max(T // 2, 1)], dtype=torch.int32)
        assert device_decode(z, il, 0) == python_decode(z, il, 0), T
        assert device_decode(z, il, 2) == python_decode(z, il, 2), T
    # C = 29 in rows of 32 whose padding holds NaN
    z = torch.randn(3, 70, 29, generator=g)
    il = torch.tensor([70, 33, 1], dtype=torch.int32)
    assert device_decode(z, il, 0, ldc=32) == python_decode(z, il, 0)
    # a class count off the 16-byte path
    z = torch.randn(2, 40, 31, generator=g)
    il = torch.tensor([40, 17], dtype=torch.int32)
    assert device_decode(z, il, 0, ldc=31) == python_decode(z, il, 0)


# ------------------------------------------------------------------------------------------------------ the letter head
from test_ctc_gpu import HOST_TOL  # noqa: E402  (f32: the kernel's bound plus the exact-f32 GEMMs; fp16: 11-bit operands)


def _float64_letter(emb, W, b, targets, tgt_len, in_len, T):
    """float64 Linear + CTC of the speech step (ref: speech_recognition_module.py:100-116) -> loss, d emb, dW, db, logits."""
    e, W, b = (t.detach().cpu().to(F64).requires_grad_(True) for t in (emb, W, b))
    U = len(tgt_len)
    logits = torch.nn.functional.linear(e, W, b).view(U, T, -1)
    lp = torch.nn.functional.log_softmax(logits, 2).transpose(0, 1)
    loss = torch.nn.functional.ctc_loss(lp, targets, in_len.to(torch.int64), tgt_len.to(torch.int64), blank=0,
                                        zero_infinity=True)
    loss.backward()
    return float(loss.detach()), e.grad, W.grad, b.grad, logits.detach()


def _rel(got, ref, k=1.0):
    got = got.detach().cpu().to(F64) / k
    return float((got - ref).norm() / ref.norm())


def _letter_head(dtype, p=0.0, train=True):
    from w2v2_speaker_amd.heads import LetterHead
    U, T, E, C = 3, 60, 24, 32
    g = torch.Generator().manual_seed(24)
    emb = torch.randn(U * T, E, generator=g).to(DEV)
    W, b = (torch.randn(C, E, generator=g) * 0.3).to(DEV), torch.randn(C, generator=g).to(DEV)
    wg, bg = torch.zeros_like(W), torch.zeros_like(b)
    scale = None if dtype == F32 else torch.tensor([256.0, 0, 0, 0, 0, 0, 0, 0], device=DEV)
    head = LetterHead(U, T, E, C, max_target=64, final_dropout=p, w_master=W, w_operand=W.to(dtype), w_grad=wg if train else None,
                      bias=b, bias_grad=bg if train else None, emb=emb, act_dtype=dtype, train=train, loss_scale=scale)
    tl = torch.tensor([40, 12, 0])
    targets = torch.randint(1, C, (U, 40), generator=g)
    for r, L in enumerate(tl.tolist()):
        targets[r, L:] = 0                                # right-padded with the blank, as the collate does
    frames = torch.tensor([60, 45, 60], dtype=torch.int32)
    return head, (emb, W, b, wg, bg), (targets, tl, frames), (U, T, E, C)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_letter_head_against_float64(dtype):
    head, (emb, W, b, wg, bg), (targets, tl, frames), (U, T, E, C) = _letter_head(dtype)
    head.set_batch(targets, tl, frames)
    loss, pred = head.forward_backward()
    torch.cuda.synchronize()
    assert pred is None and head.width == 40
    k = 1.0 if dtype == F32 else 256.0
    ref_loss, de, dW, db, logits = _float64_letter(emb, W, b, targets, tl, frames, T)
    fig = {"logits": _rel(head.logits[:, :C], logits.view(U * T, C)), "loss": abs(float(loss) - ref_loss) / max(1, abs(ref_loss)),
           "demb": _rel(head.demb, de, k), "dW": _rel(wg, dW, k), "db": _rel(bg, db, k), "bound": HOST_TOL[dtype]}
    say(f"LetterHead {dtype}", fig)
    assert max(fig["loss"], fig["logits"], fig["demb"], fig["dW"], fig["db"]) < HOST_TOL[dtype]
    # the decoder on the logits the step just produced, one copy to the host
    tokens, counts = head.decoded()
    got = [tokens[u, :int(counts[u])].tolist() for u in range(U)]
    assert got == python_decode(head.logits[:, :C].cpu().view(U, T, C), frames, 0)
    # a second batch, narrow enough for the short kernels, through the other staging buffer
    head.set_batch(targets[:, :31], torch.tensor([31, 12, 0]), frames)
    wg.zero_()
    bg.zero_()
    loss2, _ = head.forward_backward()
    ref2 = _float64_letter(emb, W, b, targets[:, :31], torch.tensor([31, 12, 0]), frames, T)
    assert head.width == 31 and abs(float(loss2) - ref2[0]) / max(1, abs(ref2[0])) < HOST_TOL[dtype]
    assert _rel(wg, ref2[2], k) < HOST_TOL[dtype]
    with pytest.raises(ValueError, match="at most 64"):
        head.set_batch(torch.ones(U, 65, dtype=torch.int64), torch.tensor([65, 1, 1]), frames)
    with pytest.raises(ValueError, match="input lengths"):
        head.set_batch(targets, tl, torch.tensor([61, 45, 60]))


def test_letter_head_final_dropout_keeps_one_mask():
    p = 0.25
    head, (emb, W, b, wg, bg), (targets, tl, frames), (U, T, E, C) = _letter_head(F32, p=p)
    head.set_batch(targets, tl, frames)
    loss, _ = head.forward_backward(seed=77)
    torch.cuda.synchronize()
    keep = head.emb != 0
    assert head.emb is not emb and 0.6 < float(keep.float().mean()) < 0.9
    assert torch.allclose(head.emb, torch.where(keep, emb / (1 - p), torch.zeros_like(emb)), rtol=1e-6, atol=0)
    # float64 from the stored operand (the dropped embedding); d(emb) is its gradient under the same mask
    ref_loss, de, dW, db, _ = _float64_letter(head.emb, W, b, targets, tl, frames, T)
    de = de * keep.cpu() / (1 - p)
    fig = {"loss": abs(float(loss) - ref_loss) / max(1, abs(ref_loss)), "demb": _rel(head.demb, de), "dW": _rel(wg, dW)}
    say("LetterHead final_dropout 0.25", fig)
    assert max(fig.values()) < HOST_TOL[F32]
    assert bool((head.demb[~keep] == 0).all())
    # an evaluation head launches no dropout: its operand is the embedding itself
    ev, _, _, _ = _letter_head(F32, p=p, train=False)
    assert ev.emb is ev.emb_in and ev.p_drop == 0.0
    ev.forward_only(frames)
    tokens, counts = ev.decoded()
    assert [int(c) >= 0 for c in counts] == [True] * U
