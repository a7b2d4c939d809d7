"""Gradient accumulation (``accumulate_grad_batches`` = N): the w2v2_grad_accumulate kernel, SpeakerTrainer and
EcapaTrainer over a window of N micro-batches, and the module surface.  The truth for the accumulated arena is torch's
f32 ``g1 + g2`` (bitwise), for a step CPU torch (clip_grad_norm_ + SGD) on the mean of the micro-batch gradients the
device produced.  Tiny configuration, 4000 samples, 10 speakers, like tests/test_optim_trainer_gpu.py.  Run with -m gpu."""
import numpy as np
import pytest
import torch

from oracle import w2v2_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
SGD = dict(momentum=0.9, nesterov=True, weight_decay=1e-4)
LR = 1e-3


def _store(dtype):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.params import ParamStore
    st = ParamStore(W2V2Config.tiny(), DEV, dtype, head="aam", num_speakers=10)
    sd = O.make_state_dict(O.OracleConfig.tiny(), 20211)
    sd["loss_fn.fc_weights"] = O.synth_tensor("loss_fn.fc_weights", (10, st.embed_dim), 20211)
    st.load_state_dict(sd)
    if st.scaler is not None:
        st.scaler[0] = 256.0          # small batches: the default scale overflows fp16 here
    return st


def _no_reg():
    from w2v2_speaker_amd.config import Wav2Vec2RegularisationConfig
    return Wav2Vec2RegularisationConfig(activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                                        hidden_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0)


def _batch():
    wav, label = O.synth_batch(4, 4000, 10, seed=3)
    return wav.to(DEV), label.to(DEV)


def _halves():
    wav, label = _batch()
    return (wav[:2], label[:2]), (wav[2:], label[2:])


def _trainer(st, batch=2, sched=None, **kw):
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    return SpeakerTrainer(st, Plan(st, batch, 4000, train=True, reg=_no_reg()), sched or Constant(LR, 0.9), **kw)


def _sgd_cfg():
    from w2v2_speaker_amd.optim import OptimConfig
    return OptimConfig("sgd", **SGD)


def _torch_sgd_step(p0, g, clip=0.0, **sgd):
    """One CPU torch step: clip_grad_norm_ (clip > 0) then SGD.  Returns the new parameters."""
    p = torch.nn.Parameter(p0.clone())
    p.grad = g.clone()
    if clip > 0:
        torch.nn.utils.clip_grad_norm_([p], clip)
    torch.optim.SGD([p], lr=LR, **(sgd or SGD)).step()
    return p.detach()


# ------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 2048, 8195, (1 << 22) + 1])
def test_grad_accumulate_kernel_matches_torch_bitwise(n):
    """n covers: tail only (1, 3), exactly one vector (4), vector + tail (5), below / at the 2 x 256-vector pass of one
    block (255, 2048), several blocks with a tail (8195) and 2^22 + 1."""
    from w2v2_speaker_amd import ops
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen).to(DEV)
    acc0 = torch.randn(n, generator=gen).to(DEV)
    g[n // 2] = float("inf")
    if n > 1:
        g[n - 1] = float("nan")
    acc = torch.full((n + 4,), float("nan"), device=DEV)      # 4 guard elements behind the slice
    acc[n:] = 7.0
    ops.grad_accumulate(acc, g, n, True)
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))     # bitwise: NaN payloads included
    assert same(acc[:n], g)
    assert bool(torch.isinf(acc[n // 2]))                      # the planted inf and NaN arrived
    assert n == 1 or bool(torch.isnan(acc[n - 1]))
    acc[:n] = acc0
    ops.grad_accumulate(acc, g, n, False)
    torch.cuda.synchronize()
    want = acc0 + g
    fin = torch.isfinite(want)
    assert torch.equal(acc[:n][fin], want[fin]) and torch.equal(torch.isnan(acc[:n]), torch.isnan(want))
    assert torch.equal(torch.isinf(acc[:n]), torch.isinf(want))
    assert bool((acc[n:] == 7.0).all())                        # nothing written past n


def test_grad_accumulate_argument_checks():
    from w2v2_speaker_amd import ops
    acc, g = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    ops.grad_accumulate(acc, g, 0, True)                       # n = 0: no launch, no error
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="grad_accumulate"):
        ops.grad_accumulate(acc[1:], g, 8, False)              # rejected by the argument check; nothing is launched
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- trainer, one process
def _window_norm(dtype, skip2):
    """Norm of the window's averaged, unscaled gradient: a probe store that only tracks the norm."""
    st = _store(dtype)
    st.track_grad_norm = True
    tr = _trainer(st, optimizer=_sgd_cfg(), accumulate_grad_batches=2)
    (w1, l1), (w2, l2) = _halves()
    tr.train_step(w1, l1, skip_layers=())
    tr.train_step(w2, l2, skip_layers=skip2)
    torch.cuda.synchronize()
    assert float(st.grad_norm[1]) == 1.0
    return float(st.grad_norm[0])


@pytest.mark.parametrize("dtype,skip2", [(torch.float32, ()), (torch.float16, ()), (torch.bfloat16, ()), (torch.float16, (1,))])
def test_two_micro_batches_step_like_torch_on_their_mean(dtype, skip2):
    """N = 2 under Nesterov SGD with weight decay and a clip at half the window's norm.  Micro-batch 1 leaves everything
    but grad_acc alone; after micro-batch 2 grad_acc is g1 + g2 bitwise and the parameters are CPU torch's on
    (g1 + g2) / (2 scale) at atol 1e-6, the bound of the single-step test next door (same kernel, same lr).  skip2 = (1,):
    LayerDrop skips layer 1 on the second micro-batch only, with stale values in that slice of grad (the partial zero_grad
    must clear them, so the layer adds zeros) and NaN all over a pre-existing grad_acc (the first micro-batch overwrites)."""
    clip = 0.5 * _window_norm(dtype, skip2)
    st = _store(dtype)
    scale = float(st.scaler[0]) if st.scaler is not None else 1.0
    st.grad_acc = torch.full_like(st.grad, float("nan"))
    tr = _trainer(st, optimizer=_sgd_cfg(), gradient_clip_val=clip, accumulate_grad_batches=2)
    n = st.n_train
    p0 = st.flat.clone()
    lp0 = st.flat_lp.clone() if st.flat_lp is not None else None
    sc0 = st.scaler.clone() if st.scaler is not None else None
    (w1, l1), (w2, l2) = _halves()
    loss1, _ = tr.train_step(w1, l1, skip_layers=())
    torch.cuda.synchronize()
    g1 = st.grad[:n].clone()
    assert tr.stepped is False and st.accum_count == 1 and tr.step == 0
    assert torch.equal(st.flat, p0) and (lp0 is None or torch.equal(st.flat_lp, lp0))
    assert st.exp_avg is None and st.exp_avg_sq is None and (st.step_head, st.step_body) == (0, 0)    # no optimiser state yet
    assert sc0 is None or torch.equal(st.scaler[:4], sc0[:4])
    assert torch.equal(st.grad_acc[:n], g1)
    buckets = {n_: (s, e) for n_, s, e in st.grad_buckets()}
    for l in skip2:
        s, e = buckets[f"layer{l}"]
        st.grad[s:e] = 3.0
    loss2, _ = tr.train_step(w2, l2, skip_layers=skip2)
    torch.cuda.synchronize()
    g2 = st.grad[:n].clone()
    for l in skip2:
        s, e = buckets[f"layer{l}"]
        assert float(g2[s:e].abs().max()) == 0.0 and torch.equal(st.grad_acc[s:e], g1[s:e])
    assert tr.stepped is True and st.accum_count == 0 and tr.step == 1
    assert torch.equal(st.grad_acc[:n], g1 + g2)
    g = ((g1 + g2) / (2 * scale)).cpu()
    want = _torch_sgd_step(p0[:n].cpu(), g, clip)
    got_norm, coef = float(st.grad_norm[0]), float(st.grad_norm[1])
    ref_norm = float(torch.linalg.vector_norm(g.double()))
    err = float((st.flat[:n].cpu() - want).abs().max())
    print(f"{dtype} skip2={skip2}: losses {float(loss1):.4f} {float(loss2):.4f} norm hip {got_norm:.6e} f64 {ref_norm:.6e} "
          f"coef {coef:.4f} max err {err:.2e}")
    assert np.isfinite(float(loss1)) and np.isfinite(float(loss2))
    assert abs(got_norm - ref_norm) <= 1e-6 * ref_norm
    assert 0.45 < coef < 0.55
    assert torch.allclose(st.flat[:n].cpu(), want, atol=1e-6, rtol=0)
    assert not torch.equal(st.flat[:n], p0[:n])
    assert torch.equal(st.flat[n:], p0[n:])                    # frozen CNN untouched
    if st.scaler is not None:
        assert float(st.scaler[3]) == 0.0
    if st.flat_lp is not None:
        assert torch.equal(st.flat_lp[:n], st.flat[:n].to(dtype))


def _plain_sgd_setup(batch, N):
    """The data-parallel tests' model and joint batch (tests/test_ddp_gpu.py) under plain SGD: no momentum, decay or clip."""
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.optim import OptimConfig
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.params import ParamStore
    st = ParamStore(W2V2Config.tiny(), DEV, torch.float32, head="aam", num_speakers=10)
    st.init_weights(seed=3)
    tr = _trainer(st, batch, Constant(LR, 0.0), optimizer=OptimConfig("sgd"), accumulate_grad_batches=N)
    wav, label = O.synth_batch(4, 4000, 10, seed=11)
    return st, tr, wav.to(DEV), label.to(DEV)


def test_accumulated_window_matches_the_joint_batch():
    """N = 2 x B = 2 against N = 1 x B = 4 on the same four utterances, f32, plain SGD, three optimiser steps: the mean of
    two half-batch means is the joint mean.  Bound: tests/test_ddp_gpu.py's for two ranks against the joint batch (the
    same arithmetic).  Plain SGD on purpose: Adam turns the rounding noise of zero-gradient elements into full steps."""
    st, tr, wav, label = _plain_sgd_setup(4, 1)
    fresh = st.flat[:st.n_train].clone()
    for _ in range(3):
        tr.train_step(wav, label, skip_layers=())
    sa, ta, _, _ = _plain_sgd_setup(2, 2)
    assert torch.equal(sa.flat[:sa.n_train], fresh)
    for _ in range(3):
        ta.train_step(wav[:2], label[:2], skip_layers=())
        ta.train_step(wav[2:], label[2:], skip_layers=())
    torch.cuda.synchronize()
    assert tr.step == ta.step == 3
    moved = float((st.flat[:st.n_train] - fresh).norm())
    err = float((sa.flat[:st.n_train] - st.flat[:st.n_train]).norm())
    print(f"accumulated vs joint batch: |dp| = {moved:.3e}, |p_acc - p_joint| = {err:.3e}")
    assert moved > 0 and err < 5e-4 * moved


def test_fp16_overflow_in_a_non_final_micro_batch_skips_the_window():
    """An inf that reaches the scanned last bucket of grad_acc during micro-batch 1 of 2 survives the addition of
    micro-batch 2: the step is skipped as a whole and the scale halved.  The next window overwrites grad_acc (first = 1),
    so it steps with everything finite."""
    from w2v2_speaker_amd.params import W2V_PREFIX
    st = _store(torch.float16)
    tr = _trainer(st, accumulate_grad_batches=2)               # default Adam, no clip: the found-inf scan decides
    (w1, l1), (w2, l2) = _halves()
    tr.train_step(w1, l1, skip_layers=())                      # a clean window first, so that the moments are non-trivial
    tr.train_step(w2, l2, skip_layers=())
    torch.cuda.synchronize()
    assert tr.stepped and float(st.scaler[3]) == 0.0
    p0, m0, v0 = st.flat.clone(), st.exp_avg.clone(), st.exp_avg_sq.clone()
    assert float(m0.abs().max()) > 0
    tr.train_step(w1, l1, skip_layers=())
    lo = st.offsets[W2V_PREFIX + "encoder.layer_norm.weight"]
    assert lo + 5 < st.n_train
    st.grad_acc[lo + 5] = float("inf")
    tr.train_step(w2, l2, skip_layers=())
    torch.cuda.synchronize()
    assert tr.stepped and st.accum_count == 0                  # the window closed (torch counts a skipped step too)
    assert torch.equal(st.flat, p0) and torch.equal(st.exp_avg, m0) and torch.equal(st.exp_avg_sq, v0)
    assert float(st.scaler[0]) == 128.0 and float(st.scaler[3]) == 1.0
    assert float(st.scaler[4]) == 1.0 and float(st.scaler[5]) == 1.0
    tr.train_step(w1, l1, skip_layers=())
    tr.train_step(w2, l2, skip_layers=())
    torch.cuda.synchronize()
    n = st.n_train
    assert bool(torch.isfinite(st.grad_acc[:n]).all()) and bool(torch.isfinite(st.flat).all())
    assert not torch.equal(st.flat[:n], p0[:n]) and float(st.scaler[3]) == 1.0


def test_default_trainer_never_accumulates():
    """Default arguments: the step issues the launches it always issued, never w2v2_grad_accumulate, and the second
    arena does not exist."""
    from w2v2_speaker_amd import ops
    st = _store(torch.float16)
    tr = _trainer(st, 4)
    assert tr.accumulate_grad_batches == 1
    calls = []
    names = ("adam_step", "optim_step", "grad_norm", "grad_scaler_check", "grad_accumulate")
    orig = {n: getattr(ops, n) for n in names}
    try:
        for n, fn in orig.items():
            setattr(ops, n, (lambda n_, fn_: lambda *a, **k: (calls.append(n_), fn_(*a, **k))[1])(n, fn))
        tr.train_step(*_batch(), skip_layers=())
        tr.flush()                                             # nothing to flush at N = 1
    finally:
        for n, fn in orig.items():
            setattr(ops, n, fn)
    assert calls == ["grad_scaler_check", "adam_step"], calls
    assert st.grad_acc is None and st.accum_count == 0 and tr.stepped is False and tr.step == 1


def test_flush_steps_on_a_partial_window_and_mixed_windows_raise():
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        _trainer(_store(torch.float32), accumulate_grad_batches=0)
    st = _store(torch.float32)
    tr = _trainer(st, optimizer=_sgd_cfg(), accumulate_grad_batches=3)
    n = st.n_train
    p0 = st.flat.clone()
    (w1, l1), (w2, l2) = _halves()
    tr.train_step(w1, l1, skip_layers=())
    g1 = st.grad[:n].clone()
    tr.train_step(w2, l2, skip_layers=())
    g2 = st.grad[:n].clone()
    torch.cuda.synchronize()
    assert not tr.stepped and st.accum_count == 2 and torch.equal(st.flat, p0)
    tr.flush()
    torch.cuda.synchronize()
    assert tr.stepped and st.accum_count == 0 and tr.step == 1
    want = _torch_sgd_step(p0[:n].cpu(), ((g1 + g2) / 3).cpu())          # PL divides by N, also in a short window
    err = float((st.flat[:n].cpu() - want).abs().max())
    print(f"flush after 2 of 3: max err {err:.2e}")
    assert torch.allclose(st.flat[:n].cpu(), want, atol=1e-6, rtol=0) and not torch.equal(st.flat[:n], p0[:n])
    p1 = st.flat.clone()
    tr.flush()                                                 # no open window: nothing happens
    torch.cuda.synchronize()
    assert torch.equal(st.flat, p1) and tr.step == 1 and not tr.stepped
    # a window holds frozen-encoder or unfrozen micro-batches, never both
    tr.train_step(w1, l1, skip_layers=())
    with pytest.raises(RuntimeError, match="frozen"):
        tr.train_step_frozen_encoder(tr.plan, w2, l2)
    tr.flush()
    tr.train_step_frozen_encoder(tr.plan, w1, l1)
    with pytest.raises(RuntimeError, match="frozen"):
        tr.train_step(w2, l2, skip_layers=())
    # ... and a frozen window steps the head slice alone, on the mean of its micro-batches
    h = st.head_size()
    p2 = st.flat.clone()
    tr.flush()
    torch.cuda.synchronize()
    assert not torch.equal(st.flat[:h], p2[:h]) and torch.equal(st.flat[h:], p2[h:]) and st.accum_count == 0


# ------------------------------------------------------------------------------------------------- ECAPA
def test_ecapa_two_micro_batches_step_like_torch_on_their_mean():
    """EcapaTrainer(accumulate_grad_batches=2) at the smallest configuration of tests/test_ecapa_gpu.py under SGD + clip:
    grad_acc = g1 + g2 bitwise, the step is CPU torch's at atol 1e-6 (the bound of the N = 1 ECAPA step of
    tests/test_optim_trainer_gpu.py), and every micro-batch moves the BatchNorm running statistics."""
    from w2v2_speaker_amd.ecapa import EcapaPlan, EcapaTrainer
    from w2v2_speaker_amd.optim.schedule import Constant
    import test_ecapa_gpu as TE
    cfg, ocfg, st, sd, feat, label = TE._setup(torch.float32)
    feat, label = feat.to(DEV), label.to(DEV)
    tr = EcapaTrainer(st, EcapaPlan(st, 2, feat.shape[1], train=True), Constant(LR, 0.9), optimizer=_sgd_cfg(),
                      gradient_clip_val=0.1, accumulate_grad_batches=2)
    running = lambda: torch.cat([r.reshape(-1) for r in st.bn_running.values()]).clone()
    p0, r0 = st.flat.clone(), running()
    tr.train_step(feat[:2], label[:2])
    torch.cuda.synchronize()
    g1, r1 = st.grad.clone(), running()
    assert not tr.stepped and st.accum_count == 1 and torch.equal(st.flat, p0) and st.exp_avg is None
    tr.train_step(feat[2:], label[2:])
    torch.cuda.synchronize()
    g2, r2 = st.grad.clone(), running()
    assert tr.stepped and st.accum_count == 0 and tr.step == 1
    assert torch.equal(st.grad_acc, g1 + g2)
    assert not torch.equal(r0, r1) and not torch.equal(r1, r2)
    g = ((g1 + g2) / 2).cpu()
    want = _torch_sgd_step(p0.cpu(), g, 0.1)
    ref_norm = float(torch.linalg.vector_norm(g.double()))
    print(f"ecapa N=2: norm hip {float(st.grad_norm[0]):.6e} f64 {ref_norm:.6e} coef {float(st.grad_norm[1]):.4f} "
          f"max err {float((st.flat.cpu() - want).abs().max()):.2e}")
    assert abs(float(st.grad_norm[0]) - ref_norm) <= 1e-6 * ref_norm
    assert float(st.grad_norm[1]) < 1.0
    assert torch.allclose(st.flat.cpu(), want, atol=1e-6, rtol=0)
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        EcapaTrainer(st, tr.plan, Constant(LR, 0.9), accumulate_grad_batches=0)


# ------------------------------------------------------------------------------------------------- module surface
def _fc_module(frozen_steps=None, **kw):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import Wav2vec2FCModule, Wav2vec2FCModuleConfig
    tiny = W2V2Config.tiny()
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: tiny)
    mcfg = Wav2vec2FCModuleConfig(reset_weights=True, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                                  hidden_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0,
                                  wav2vec_initially_frozen=frozen_steps is not None, num_frozen_steps=frozen_steps)
    try:
        return Wav2vec2FCModule.from_config(mcfg, num_speakers=10, device=DEV, act_dtype=torch.float32, init_seed=5,
                                            max_lr=1e-3, max_steps=20, **kw)
    finally:
        W2V2Config.from_huggingface_id = orig


def test_fc_module_steps_every_second_call_and_guards_the_window(tmp_path):
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import SpeakerClassificationDataBatch
    wav, label = O.synth_batch(4, 4000, 10, seed=3)
    batch = SpeakerClassificationDataBatch(4, list("abcd"), wav, label).to(DEV)
    mod = _fc_module(accumulate_grad_batches=2)
    mod.train()
    mod.on_train_start()
    changed, sched = [], []
    for i in range(4):
        before = mod.store.flat.clone()
        out = mod.training_step(batch, i)
        torch.cuda.synchronize()
        changed.append(not torch.equal(mod.store.flat, before))
        sched.append(mod.schedule_step)
        assert np.isfinite(float(out["loss"]))
    assert changed == [False, True, False, True] and sched == [0, 1, 1, 2] and mod.steps == 4
    # inside a window no checkpoint is written; the end of the epoch flushes it
    mod.training_step(batch, 4)
    assert mod.store.accum_count == 1 and mod.steps == 5
    path = str(tmp_path / "accum.ckpt")
    with pytest.raises(RuntimeError, match="flush"):
        mod.save_checkpoint(path)
    before = mod.store.flat.clone()
    mod.on_train_epoch_end()
    torch.cuda.synchronize()
    assert mod.store.accum_count == 0 and mod.schedule_step == 3 and not torch.equal(mod.store.flat, before)
    mod.save_checkpoint(path)
    assert torch.load(path, weights_only=False)["global_step"] == 3
    mod.on_train_epoch_end()                                   # no open window: nothing happens
    assert mod.schedule_step == 3
    # the unfreeze may not fall inside a window
    with pytest.raises(ValueError, match="num_frozen_steps"):
        _fc_module(frozen_steps=3, accumulate_grad_batches=2)
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        _fc_module(accumulate_grad_batches=0)
    fm = _fc_module(frozen_steps=2, accumulate_grad_batches=2)
    fm.train()
    fm.on_train_start()
    h = fm.store.head_size()
    p0 = fm.store.flat.clone()
    for i in range(2):
        fm.training_step(batch, i)                             # one frozen window: the head moves, the encoder does not
    torch.cuda.synchronize()
    assert fm.schedule_step == 1 and not fm._is_wav2vec_frozen
    assert not torch.equal(fm.store.flat[:h], p0[:h]) and torch.equal(fm.store.flat[h:], p0[h:])
    for i in range(2):
        fm.training_step(batch, 2 + i)                         # unfrozen from the first micro-batch of the next window
    torch.cuda.synchronize()
    assert fm.schedule_step == 2 and not torch.equal(fm.store.flat[h:fm.store.n_train], p0[h:fm.store.n_train])


def test_ecapa_and_paired_modules_accept_the_keyword():
    from w2v2_speaker_amd import config as C
    from w2v2_speaker_amd.lightning_modules.speaker.ecapa_tdnn import EcapaTDNNModuleConfig, EcapaTdnnModule
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import SpeakerClassificationDataBatch
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_paired_input import (
        PairedSpeakerClassificationDataBatch, Wav2vec2PairedSpeakerModule, Wav2vec2PairedSpeakerModuleConfig)
    from w2v2_speaker_amd.optim.loss import AngularAdditiveMarginSoftMaxLoss, BinaryCrossEntropyLoss
    g = torch.Generator().manual_seed(0)
    ecfg = EcapaTDNNModuleConfig(input_mel_coefficients=16, lin_neurons=24, channels=[64, 64, 64, 64, 192],
                                 attention_channels=16, res2net_scale=4, se_channels=16)
    actor = lambda: AngularAdditiveMarginSoftMaxLoss(2, 2, margin=0.2, scale=30.0, device=DEV, act_dtype=torch.float32)
    em = EcapaTdnnModule(None, ecfg, 5, actor, [], [], None, accumulate_grad_batches=2)
    feat = torch.randn(6, 40, 16, generator=g)
    batch = SpeakerClassificationDataBatch(6, [str(i) for i in range(6)], feat, torch.randint(0, 5, (6,), generator=g))
    p0 = em.store.flat.clone()
    em.training_step(batch)
    torch.cuda.synchronize()
    assert em.schedule_step == 0 and em.steps == 1 and torch.equal(em.store.flat, p0)
    em.training_step(batch)
    torch.cuda.synchronize()
    assert em.schedule_step == 1 and em.steps == 2 and not torch.equal(em.store.flat, p0)
    em.training_step(batch)
    em.on_train_epoch_end()
    assert em.schedule_step == 2 and em.store.accum_count == 0
    tiny = C.W2V2Config.tiny()
    orig = C.W2V2Config.from_huggingface_id
    C.W2V2Config.from_huggingface_id = staticmethod(lambda _id: tiny)
    try:
        pm = Wav2vec2PairedSpeakerModule(None, Wav2vec2PairedSpeakerModuleConfig(), BinaryCrossEntropyLoss,
                                         accumulate_grad_batches=2)
    finally:
        C.W2V2Config.from_huggingface_id = orig
    pm.store.scaler[0] = 256.0
    a, b = 0.3 * torch.randn(4, 4000, generator=g), 0.3 * torch.randn(4, 4000, generator=g)
    pb = PairedSpeakerClassificationDataBatch(4, list("abcd"), a, list("efgh"), b, torch.tensor([1, 0, 1, 0]))
    p0 = pm.store.flat.clone()
    pm.training_step(pb)
    torch.cuda.synchronize()
    assert pm.schedule_step == 0 and pm.steps == 1 and torch.equal(pm.store.flat, p0)
    pm.training_step(pb)
    torch.cuda.synchronize()
    assert pm.schedule_step == 1 and pm.steps == 2 and not torch.equal(pm.store.flat, p0)
    assert float(pm.store.scaler[3]) == 0.0
