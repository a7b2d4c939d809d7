"""GPU tests of the CTC loss: the kernels (w2v2_ctc_fwd_bwd) against the float64 reference of tests/ctc_cases.py,
heads.CtcHead, the CtcLoss module against gradients the reference's own class produced (tests/golden/g22_ctc.npz), and
the "ctc" mode of Plan, SpeakerTrainer and Wav2vec2FCModule.

Bounds (tests/ctc_cases.py): loss rows 2e-5 relative to max(1, |ref|); gradient rel-L2 per utterance, the largest over the
batch, at most max(1e-5, 2 x the error of torch's own f32 CPU F.ctc_loss on the same inputs).  tests/test_ctc_cpu.py
shows that the kernel's arithmetic restated in f32 on the CPU meets them, so a miss here is the kernel's.  Lines that
start with ``ctc-parity:`` are the measured figures recorded in profiles/ctc_parity.txt."""
import os

import numpy as np
import pytest
import torch

import ctc_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
SENT = -7.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def ops():
    from w2v2_speaker_amd import ops as o
    return o


def say(what, figures):
    print("ctc-parity: " + what + ": " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}"
                                                     for k, v in figures.items()))


def device_logits(c):
    """[B*T, ldc] f32 on the device, NaN in the padding columns."""
    B, T, C = c["logits"].shape
    z = torch.full((B * T, c["ldc"]), float("nan"), dtype=F32)
    z[:, :C] = c["logits"].reshape(B * T, C)
    return z.to(DEV)


def launch(c, *, grad=F32, loss_scale=None, targets=None, tgt_len=None, in_len=None, offset=0, logits=None):
    """One launch into sentinel-filled outputs -> (loss_rows [B], dlogits [B, T, ldc] or None), device tensors."""
    o = ops()
    B, T, C = c["logits"].shape
    ldc = c["ldc"]
    z = device_logits(c) if logits is None else logits
    tg = (c["targets"] if targets is None else targets).to(DEV)
    il = (c["in_len"] if in_len is None else in_len).to(DEV)
    tl = (c["tgt_len"] if tgt_len is None else tgt_len).to(DEV)
    rows = torch.full((B,), SENT, dtype=F32, device=DEV)
    dl = None if grad is None else torch.full((B * T, ldc), SENT, dtype=grad, device=DEV)
    ws = torch.full((o.ctc_workspace_floats(B, T, tg.shape[1]),), float("nan"), dtype=F32, device=DEV)
    ls = None if loss_scale is None else torch.tensor([loss_scale, 0.0, 0.0, 0.0], device=DEV)
    o.ctc_fwd_bwd(z, tg, il, tl, rows, dl, ws, B, T, C, ldc, target_width=tg.shape[1], target_offset=offset,
                  blank=c["blank"], loss_scale=ls)
    torch.cuda.synchronize()
    return rows, None if dl is None else dl.view(B, T, ldc)


@pytest.mark.parametrize("name", CC.CASES)
def test_kernel_against_float64(name):
    c = CC.case(name)
    C = c["logits"].shape[2]
    rows, dl = launch(c)
    assert bool((dl[..., C:] == SENT).all()), "the padding columns are not the kernel's to write"
    e = CC.errors(c, rows, dl[..., :C])
    say(name, {**e, "bound": CC.grad_bound(name), "torch_f32": CC.ref_f32_error(name)})
    assert e["loss_rows"] < CC.LOSS_TOL
    assert e["grad"] <= CC.grad_bound(name)
    assert e["zeros_ok"], "infeasible utterances and frames past an utterance's end get exact zeros"
    # sum_c dlogits[t, :] of a live frame is zero to rounding (softmax and posteriors both sum to one): a few ulp of the
    # O(1 / B) terms; times B in errors()
    assert e["row_sum"] < 2e-5
    for b in c["infinite"]:
        assert float(rows[b]) == 0.0


def test_two_launches_are_bitwise_equal():
    for name in ("mixed", "repeats", "c1021_nan_padding"):
        c = CC.case(name)
        C = c["logits"].shape[2]
        r1, d1 = launch(c)
        r2, d2 = launch(c)
        assert torch.equal(r1, r2) and torch.equal(d1[..., :C], d2[..., :C])


def test_forward_only_leaves_the_gradient_alone():
    c = CC.case("mixed")
    rows_fb, _ = launch(c)
    rows, none = launch(c, grad=None)
    assert none is None and torch.equal(rows, rows_fb)


def test_loss_scale_weighs_the_gradient_only():
    c = CC.case("full_lattice")
    C = c["logits"].shape[2]
    r1, d1 = launch(c)
    r2, d2 = launch(c, loss_scale=1024.0)
    assert torch.equal(r1, r2)
    assert torch.equal(d2[..., :C], d1[..., :C] * 1024.0)        # a power of two: exact


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16_bit_gradient_is_the_f32_one_rounded(dtype):
    for name, scale in (("mixed", 256.0), ("c1021_nan_padding", 1.0), ("c257", 1.0)):
        c = CC.case(name)
        C = c["logits"].shape[2]
        _, d32 = launch(c, loss_scale=scale)
        _, d16 = launch(c, grad=dtype, loss_scale=scale)
        assert torch.equal(d16[..., :C], d32[..., :C].to(dtype))
        assert bool((d16[..., C:] == SENT).all())


def test_target_offset_shifts_the_class():
    c = CC.case("mixed")
    C = c["logits"].shape[2]
    r1, d1 = launch(c)
    r2, d2 = launch(c, targets=c["targets"] - 1, offset=1)
    assert torch.equal(r1, r2) and torch.equal(d1[..., :C], d2[..., :C])


def test_bad_rows_are_nan_with_zero_gradients():
    """A target outside [0, C), the blank as a target, a target length beyond the row width, an input length beyond T: NaN
    loss row, zero gradient, the good rows as before (nothing out of range is read: the targets of the bad rows point
    far outside the logits)."""
    c = CC.case("mixed")
    B, T, C = c["logits"].shape
    good_rows, good = launch(c)
    for what in ("class_high", "class_negative", "blank", "target_length", "input_length"):
        tg, tl, il = c["targets"].clone(), c["tgt_len"].clone(), c["in_len"].clone()
        if what == "class_high":
            tg[1, 3] = C + (1 << 40)
        elif what == "class_negative":
            tg[1, 0] = -(1 << 40)
        elif what == "blank":
            tg[1, 2] = c["blank"]
        elif what == "target_length":
            tl[1] = tg.shape[1] + 1
        else:
            il[1] = T + 1
        rows, dl = launch(c, targets=tg, tgt_len=tl, in_len=il)
        assert bool(torch.isnan(rows[1])), what
        assert bool((dl[1, :, :C] == 0).all()), what
        keep = [0, 2, 3]
        assert torch.equal(rows[keep], good_rows[keep]) and torch.equal(dl[keep][..., :C], good[keep][..., :C]), what
    # a bad class beyond a row's target length is padding, not an error
    tg = c["targets"].clone()
    tg[2, 5] = -5
    rows, dl = launch(c, targets=tg)
    assert torch.equal(rows, good_rows) and torch.equal(dl[..., :C], good[..., :C])


def test_width_limit_is_a_host_error():
    c = CC.case("one_frame")
    with pytest.raises(ValueError):
        launch(c, targets=torch.ones(2, 32, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------------ host layers
from oracle import w2v2_oracle as O  # noqa: E402

B, N, SPK = 4, 4000, 5            # tiny config, 4 utterances of 4000 samples (12 frames), 5 speakers + the blank
ENC = "encoder.layers.1.feed_forward.output_dense.weight"
W_HEAD, B_HEAD = "fc_list.0.0.weight", "fc_list.0.0.bias"
# f32: the kernel's bound plus the rounding of the exact-f32 GEMMs behind it.  fp16: the operands of the three head GEMMs
# are rounded to 11 bits (4.9e-4 each): the figure __graft_entry__.smoke() holds the fp16 mode to
HOST_TOL = {torch.float32: 2e-5, torch.float16: 3e-3}


def _reg():
    from w2v2_speaker_amd.config import Wav2Vec2RegularisationConfig
    return Wav2Vec2RegularisationConfig(activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                                        hidden_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0)


def _store(dtype, head="ctc"):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.params import ParamStore
    cfg = W2V2Config.tiny()
    st = ParamStore(cfg, DEV, dtype, head=head, num_speakers=SPK, embed_dim=cfg.hidden_size)
    sd = O.make_state_dict(O.OracleConfig.tiny(), 20211)
    rows = SPK + 1 if head == "ctc" else SPK
    sd[W_HEAD] = O.synth_tensor(W_HEAD, (rows, cfg.hidden_size), 20211)
    sd[B_HEAD] = O.synth_tensor(B_HEAD, (rows,), 20211)
    st.load_state_dict(sd)
    if st.scaler is not None:
        st.scaler[0] = 256.0
    return st


def _plan(st):
    from w2v2_speaker_amd.engine import Plan
    return Plan(st, B, N, train=True, reg=_reg(), pooling="none")


def _batch():
    wav, _ = O.synth_batch(B, N, SPK, seed=5)
    return wav, torch.tensor([0, 4, 3, 3], dtype=torch.int64)


def _float64_head(emb, W, b, label, T):
    """float64 Linear + CTC of the speaker step (ref: speaker_recognition_module.py:222-244) -> loss, d emb, dW, db."""
    e, W, b = (t.detach().cpu().to(F64).requires_grad_(True) for t in (emb, W, b))
    logits = torch.nn.functional.linear(e, W, b).view(len(label), T, -1)
    lp = torch.nn.functional.log_softmax(logits, 2).transpose(0, 1)
    loss = torch.nn.functional.ctc_loss(lp, (label + 1)[:, None], torch.full((len(label),), T), torch.ones(len(label), dtype=torch.int64),
                                        blank=0, zero_infinity=True)
    loss.backward()
    return float(loss.detach()), e.grad, W.grad, b.grad, logits.detach()


def _rel(got, ref, k=1.0):
    got = got.detach().cpu().to(F64) / k
    return float((got - ref).norm() / ref.norm())


def test_ctc_head_against_the_kernel_and_float64_linear():
    """heads.CtcHead on its own: logits = F.linear, loss and d(logits) the kernel's, d emb / dW / db the float64 ones."""
    from w2v2_speaker_amd.heads import CtcHead
    U, T, E, C = 3, 7, 24, 11
    g = torch.Generator().manual_seed(9)
    emb = torch.randn(U * T, E, generator=g).to(DEV)
    W, b = (torch.randn(C, E, generator=g) * 0.3).to(DEV), torch.randn(C, generator=g).to(DEV)
    wg, bg = torch.zeros_like(W), torch.zeros_like(b)
    label = torch.tensor([9, 0, 4], device=DEV)
    head = CtcHead(U, T, E, C, w_master=W, w_operand=W, w_grad=wg, bias=b, bias_grad=bg, emb=emb, act_dtype=F32, train=True)
    loss, pred = head.forward_backward(label)
    torch.cuda.synchronize()
    assert pred is None and label.tolist() == [9, 0, 4]
    ref_loss, de, dW, db, logits = _float64_head(emb, W, b, label.cpu(), T)
    fig = {"logits": _rel(head.logits[:, :C], logits.view(U * T, C)), "loss": abs(float(loss) - ref_loss) / max(1, abs(ref_loss)),
           "demb": _rel(head.demb, de), "dW": _rel(wg, dW), "db": _rel(bg, db)}
    say("CtcHead f32", fig)
    assert fig["loss"] < CC.LOSS_TOL and max(fig["logits"], fig["demb"], fig["dW"], fig["db"]) < HOST_TOL[F32]
    # the gradient operand is the kernel's own output on the head's logits
    c = {"logits": head.logits[:, :C].cpu().view(U, T, C), "ldc": head.ldc, "blank": 0,
         "targets": (label.cpu() + 1)[:, None], "in_len": torch.full((U,), T, dtype=torch.int32),
         "tgt_len": torch.ones(U, dtype=torch.int32)}
    z = torch.zeros(U * T, head.ldc, device=DEV)
    z[:, :C] = head.logits[:, :C]
    rows, dl = launch(c, logits=z)
    assert torch.equal(rows, head.loss_rows) and torch.equal(dl.view(U * T, -1)[:, :C], head.dcos_w[:, :C])
    # an evaluation head touches no gradient
    ev = CtcHead(U, T, E, C, w_master=W, w_operand=W, w_grad=None, bias=b, bias_grad=None, emb=emb, act_dtype=F32, train=False)
    l2, _ = ev.forward_backward(label)
    assert float(l2) == float(loss) and not hasattr(ev, "dcos_w")


def test_ctc_loss_module_gives_the_reference_gradients():
    from w2v2_speaker_amd.optim.loss import CtcLoss
    g = np.load(os.path.join(GOLDEN, "g22_ctc.npz"))
    t = lambda k: torch.from_numpy(g[k])
    for layout, targets in (("2d", t("generic_targets")), ("1d", t("generic_targets_1d"))):
        for dtype in (F32, torch.float16, torch.bfloat16):
            x = t("generic_logits").to(dtype).to(DEV).requires_grad_(True)
            loss = CtcLoss()(x, t("generic_in_len").to(DEV), targets.to(DEV), t("generic_tgt_len").to(DEV))
            (loss * 3.0).backward()
            assert loss.dtype == dtype and x.grad.dtype == dtype and x.grad.shape == x.shape
            if dtype == F32:
                fig = {"loss": abs(float(loss) - float(g[f"generic_{layout}_loss"])) / max(1.0, float(g[f"generic_{layout}_loss"])),
                       "grad": CC.per_utterance_rel_l2(x.grad / 3.0, t(f"generic_{layout}_grad"))}
                say(f"CtcLoss {layout}", fig)
                assert fig["loss"] < CC.LOSS_TOL and fig["grad"] < CC.GRAD_TOL
                assert bool((x.grad[4] == 0).all())                         # the infeasible utterance
            else:       # the same kernel on the rounded predictions: compare with float64 on those
                ref = CC.ctc_ref(x.detach().cpu().float(), t("generic_targets"), t("generic_in_len"), t("generic_tgt_len"))
                eps = 2.0 ** (-10 if dtype == torch.float16 else -7)        # loss and gradient come back in `dtype`
                assert abs(float(loss) - float(ref["loss"])) < eps * float(ref["loss"])
                assert CC.per_utterance_rel_l2(x.grad.float() / 3.0, ref["grad"]) < eps
    # the speaker step of the reference, lengths on the host as it builds them
    x = t("step_logits").float().to(DEV).requires_grad_(True)
    U, T, _ = x.shape
    loss = CtcLoss()(x, (torch.ones(U) * T).to(torch.int32), (t("step_label") + 1).to(DEV), torch.ones(U).to(torch.int32))
    loss.backward()
    assert abs(float(loss) - float(g["step_loss"])) < CC.LOSS_TOL * float(g["step_loss"])
    assert CC.per_utterance_rel_l2(x.grad, t("step_grad")) < CC.GRAD_TOL
    with pytest.raises(ValueError, match="at most 31"):
        CtcLoss()(x, torch.ones(U), torch.ones(U, 32, dtype=torch.int64), torch.ones(U))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_plan_gradients(dtype):
    """The plan's head gradients against float64 Linear + CTC composed on the plan's own last hidden state (the [B*T, H]
    embedding of the no-pooling plan); fp16: on gradient / loss_scale."""
    wav, label = _batch()
    st = _store(dtype)
    plan = _plan(st)
    plan.embed(wav.to(DEV), None, (), 0)
    dev_label = label.to(DEV)
    loss, pred = plan.head_forward_backward(dev_label)
    torch.cuda.synchronize()
    assert pred is None and torch.equal(dev_label.cpu(), label) and plan.head_rows == B * plan.T
    k = 1.0 if st.scaler is None else float(st.scaler[0])
    ref_loss, de, dW, db, _ = _float64_head(plan.emb, st.p(W_HEAD), st.p(B_HEAD), label, plan.T)
    fig = {"loss": abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss)), "demb": _rel(plan.demb, de, k),
           "dW": _rel(st.g(W_HEAD), dW, k), "db": _rel(st.g(B_HEAD), db, k), "bound": HOST_TOL[dtype]}
    say(f"plan ctc {dtype}", fig)
    assert max(fig["loss"], fig["demb"], fig["dW"], fig["db"]) < HOST_TOL[dtype]
    with pytest.raises(ValueError, match="triplets were given"):
        plan.head_forward_backward(dev_label, ([1, 0, 3, 2], [2, 3, 0, 1]))
    from w2v2_speaker_amd.engine import Plan
    with pytest.raises(ValueError, match="speaker_wav2vec2_ctc"):
        Plan(st, B, N, train=True, reg=_reg(), pooling="mean+std")
    ev = Plan(st, B, N, train=False, reg=_reg(), pooling="mean+std")          # evaluation plans are unaffected
    assert tuple(ev.embed(wav.to(DEV)).shape) == (B, 2 * st.cfg.hidden_size) and ev.head is None


def _trainer(accumulate=1, **kw):
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    st = _store(torch.float32)
    plan = _plan(st)
    return st, plan, SpeakerTrainer(st, plan, Constant(1e-3), accumulate_grad_batches=accumulate, **kw)


def test_train_steps_lower_the_loss():
    wav, label = _batch()
    st, plan, tr = _trainer(gradient_clip_val=5.0)
    before, head_before = st.mp(ENC).clone(), st.p(W_HEAD).clone()
    losses = []
    for _ in range(6):
        loss, pred = tr.train_step(wav.to(DEV), label.to(DEV), skip_layers=())
        losses.append(float(loss))
        assert pred is None
        if len(losses) == 1:
            assert not torch.equal(st.mp(ENC), before) and not torch.equal(st.p(W_HEAD), head_before)
    torch.cuda.synchronize()
    say("trainer ctc six steps", {"first": losses[0], "last": losses[-1]})
    assert bool(torch.isfinite(st.flat).all()) and np.isfinite(losses).all() and losses[-1] < losses[0]
    assert st.step_head == st.step_body == 6


def test_sgd_steps_lower_the_loss():
    from w2v2_speaker_amd.optim import OptimConfig
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    wav, label = _batch()
    st = _store(torch.float32)
    plan = _plan(st)
    tr = SpeakerTrainer(st, plan, Constant(1e-2), optimizer=OptimConfig(algo="sgd", momentum=0.9))
    losses = [float(tr.train_step(wav.to(DEV), label.to(DEV), skip_layers=())[0]) for _ in range(6)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0]


def test_accumulation_window_and_frozen_encoder():
    wav, label = _batch()
    st, plan, tr = _trainer(accumulate=2)
    before = st.mp(ENC).clone()
    tr.train_step(wav.to(DEV), label.to(DEV), skip_layers=())
    assert not tr.stepped and torch.equal(st.mp(ENC), before)
    tr.train_step(wav.to(DEV), label.to(DEV), skip_layers=())
    assert tr.stepped and not torch.equal(st.mp(ENC), before)
    st, plan, tr = _trainer()
    flat = st.flat.clone()
    loss, pred = tr.train_step_frozen_encoder(plan, wav.to(DEV), label.to(DEV))
    torch.cuda.synchronize()
    h = st.head_size()
    assert np.isfinite(float(loss)) and pred is None and h > 0
    assert torch.equal(st.flat[h:], flat[h:]) and not torch.equal(st.flat[:h], flat[:h])
    assert (st.step_head, st.step_body) == (1, 0)


def test_module(tmp_path):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import (SpeakerClassificationDataBatch, Wav2vec2FCModule,
                                                                        Wav2vec2FCModuleConfig)
    from w2v2_speaker_amd.optim.loss import CtcLoss
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: W2V2Config.tiny())
    try:
        # config/experiment/speaker_wav2vec2_ctc.yaml: no pooling in training, mean+std in evaluation
        cfg = Wav2vec2FCModuleConfig(reset_weights=True, attention_dropout=0.0, feat_proj_dropout=0.0, hidden_dropout=0.0,
                                     layerdrop=0.0, mask_time_prob=0.0, stat_pooling_type="none",
                                     test_stat_pooling_type="mean+std")
        kw = dict(device=DEV, act_dtype=torch.float32, max_lr=1e-3, max_steps=50)
        mod = Wav2vec2FCModule.from_config(cfg, num_speakers=SPK, loss="ctc", **kw)
        H = mod.model_cfg.hidden_size
        assert mod.loss == "ctc" and mod.num_speakers == SPK + 1            # ref: speaker_recognition_module.py:104-107
        assert tuple(mod.store.p(W_HEAD).shape) == (SPK + 1, H)
        assert mod.store.p(B_HEAD).tolist() == [100.0] + [0.0] * SPK        # ref: wav2vec2_fc.py:226-233
        wav, label = _batch()
        kept = label.clone()
        batch = SpeakerClassificationDataBatch(B, list("abcd"), wav, label)
        mod.train()
        mod.on_train_start()
        before = mod.store.mp(ENC).clone()
        out = mod.training_step(batch)
        assert set(out) == {"loss", "prediction", "train_acc"} and np.isfinite(float(out["loss"]))
        assert out["prediction"] is None and out["train_acc"] is None
        assert not torch.equal(mod.store.mp(ENC), before)
        assert torch.equal(batch.ground_truth, kept) and torch.equal(label, kept)      # the reference adds 1 in place
        first = float(out["loss"])
        for _ in range(4):
            out = mod.training_step(batch)
        assert float(out["loss"]) < first
        mod.eval()
        emb = mod.compute_speaker_embedding(wav)      # (forward() would feed 2H features to the Linear, as in the reference)
        assert tuple(emb.shape) == (B, 2 * H)                                # test_stat_pooling_type: mean+std
        frames = torch.randn(B, 12, H, device=DEV)
        assert tuple(mod.compute_speaker_prediction(frames).shape) == (B, 12, SPK + 1)
        path = str(tmp_path / "ctc.ckpt")
        mod.save_checkpoint(path)
        sd = torch.load(path, map_location="cpu", weights_only=True)["state_dict"]
        assert tuple(sd[W_HEAD].shape) == (SPK + 1, H) and tuple(sd[B_HEAD].shape) == (SPK + 1,)
        back = Wav2vec2FCModule.load_from_checkpoint(path, cfg=cfg, num_speakers=SPK, loss_fn_constructor=CtcLoss, **kw)
        assert back.loss == "ctc" and torch.equal(back.store.flat, mod.store.flat)
        assert back.store.step_body == mod.store.step_body == 5
        # no pooling in evaluation too: [B, T, H] embeddings and [B, T, C + 1] predictions
        cfg2 = Wav2vec2FCModuleConfig(reset_weights=True, stat_pooling_type="none", test_stat_pooling_type="none")
        m2 = Wav2vec2FCModule.from_config(cfg2, num_speakers=SPK, loss="ctc", **kw)
        m2.eval()
        emb, pred = m2.forward(wav)
        assert tuple(emb.shape) == (B, 12, H) and tuple(pred.shape) == (B, 12, SPK + 1)
        # explicit_num_speakers is taken as it is (ref: wav2vec2_fc.py:199-210)
        cfg3 = Wav2vec2FCModuleConfig(reset_weights=True, stat_pooling_type="none", explicit_num_speakers=9)
        assert tuple(Wav2vec2FCModule.from_config(cfg3, num_speakers=SPK, loss="ctc", **kw).store.p(W_HEAD).shape) == (9, H)
    finally:
        W2V2Config.from_huggingface_id = orig
