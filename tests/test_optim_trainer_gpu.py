"""Engine-level tests of the optimiser options: SGD / weight decay / gradient-norm clipping / tri-stage through
SpeakerTrainer, EcapaTrainer, the checkpoint format and the Lightning-style module surface.  The truth for a step is
CPU torch (torch.optim.SGD + torch.nn.utils.clip_grad_norm_) applied to the gradient the device produced.  Tiny
configuration, batch 4, 4000 samples, 10 speakers, like the neighbouring Adam test.  Run with -m gpu."""
import numpy as np
import pytest
import torch

from oracle import w2v2_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
SGD = dict(momentum=0.9, nesterov=True, weight_decay=1e-4)


def _cfgs():
    from w2v2_speaker_amd.config import W2V2Config
    return W2V2Config.tiny(), O.OracleConfig.tiny()


def _store(dtype):
    from w2v2_speaker_amd.params import ParamStore
    cfg, ocfg = _cfgs()
    st = ParamStore(cfg, DEV, dtype, head="aam", num_speakers=10)
    sd = O.make_state_dict(ocfg, 20211)
    sd["loss_fn.fc_weights"] = O.synth_tensor("loss_fn.fc_weights", (10, st.embed_dim), 20211)
    st.load_state_dict(sd)
    if st.scaler is not None:
        st.scaler[0] = 256.0          # B = 4: d loss / d cos is 16x the workload's; the default scale overflows fp16 here
    return st


def _no_reg():
    from w2v2_speaker_amd.config import Wav2Vec2RegularisationConfig
    return Wav2Vec2RegularisationConfig(activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                                        hidden_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0)


def _batch():
    wav, label = O.synth_batch(4, 4000, 10, seed=3)
    return wav.to(DEV), label.to(DEV)


def _sgd_cfg():
    from w2v2_speaker_amd.optim import OptimConfig
    return OptimConfig("sgd", **SGD)


def _torch_sgd_step(p0, g, clip, lr=1e-3):
    """One CPU torch step: clip_grad_norm_ then SGD.  Returns (new parameters, the norm clip_grad_norm_ measured)."""
    p = torch.nn.Parameter(p0.clone())
    p.grad = g.clone()
    norm = torch.nn.utils.clip_grad_norm_([p], clip)
    torch.optim.SGD([p], lr=lr, **SGD).step()
    return p.detach(), float(norm)


def _plant_stale(st, skip_layers):
    """A previous step's leftovers in the gradient slice of every layer that this step skips."""
    buckets = {n: (s, e) for n, s, e in st.grad_buckets()}
    for l in skip_layers:
        s, e = buckets[f"layer{l}"]
        st.grad[s:e] = 3.0


def _measured_norm(dtype, skip_layers=()):
    """Norm of the first step's unscaled gradient: a probe store that only tracks the norm."""
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    st = _store(dtype)
    st.track_grad_norm = True
    _plant_stale(st, skip_layers)
    tr = SpeakerTrainer(st, Plan(st, 4, 4000, train=True, reg=_no_reg()), Constant(1e-3, 0.9), optimizer=_sgd_cfg())
    tr.train_step(*_batch(), skip_layers=skip_layers)
    torch.cuda.synchronize()
    assert float(st.grad_norm[1]) == 1.0                  # tracking does not clip
    return float(st.grad_norm[0])


@pytest.mark.parametrize("dtype,skip", [(torch.float32, ()), (torch.float16, ()), (torch.bfloat16, (1,)), (torch.float16, (1,))])
def test_sgd_clip_decay_step_matches_torch(dtype, skip):
    """One train_step under Nesterov SGD with weight decay 1e-4 and a clip value of half the measured norm == CPU torch
    on the device's own gradient (atol 1e-6, the Adam test's bound); the frozen CNN is untouched; grad_norm[0] is the
    norm of the unscaled arena to 1e-6 relative.  skip = (1,) in a 16-bit mode takes the partial zero_grad path: the
    arena is coherent only because the skipped layer's slice was zeroed, which the norm pins."""
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    clip = 0.5 * _measured_norm(dtype, skip)
    st = _store(dtype)
    scale = float(st.scaler[0]) if st.scaler is not None else 1.0
    _plant_stale(st, skip)               # the partial zero_grad must clear them
    tr = SpeakerTrainer(st, Plan(st, 4, 4000, train=True, reg=_no_reg()), Constant(1e-3, 0.9), optimizer=_sgd_cfg(),
                        gradient_clip_val=clip)
    p0 = st.flat.clone()
    loss, _ = tr.train_step(*_batch(), skip_layers=skip)
    torch.cuda.synchronize()
    n = st.n_train
    g = st.grad[:n].cpu() / scale
    want, norm = _torch_sgd_step(p0[:n].cpu(), g, clip)
    got_norm, coef = float(st.grad_norm[0]), float(st.grad_norm[1])
    err = float((st.flat[:n].cpu() - want).abs().max())
    print(f"{dtype} skip={skip}: loss {float(loss):.4f} norm hip {got_norm:.6e} torch {norm:.6e} coef {coef:.4f} max err {err:.2e}")
    assert np.isfinite(float(loss))
    for l in skip:
        lo, hi = {n_: (s, e) for n_, s, e in st.grad_buckets()}[f"layer{l}"]
        assert float(st.grad[lo:hi].abs().max()) == 0.0
    assert abs(got_norm - float(torch.linalg.vector_norm(g.double()))) <= 1e-6 * got_norm
    assert 0.45 < coef < 0.55
    assert torch.allclose(st.flat[:n].cpu(), want, atol=1e-6, rtol=0)
    assert not torch.equal(st.flat[:n], p0[:n])
    assert torch.equal(st.flat[n:], p0[n:])               # frozen CNN untouched
    assert st.exp_avg_sq is None                          # SGD allocates one state arena
    if st.scaler is not None:
        assert float(st.scaler[3]) == 0.0                 # nothing skipped
    if st.flat_lp is not None:
        assert torch.equal(st.flat_lp[:n], st.flat[:n].to(dtype))


def test_head_only_step_clips_over_the_head_slice():
    """train_step_frozen_encoder with clipping: the norm covers the head slice alone (large values planted in the body
    gradient after the head's backward must not enter it) and the body is bit-unchanged."""
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    st = _store(torch.float32)
    plan = Plan(st, 4, 4000, train=True, reg=_no_reg())
    h = st.head_size()
    assert 0 < h < st.n_train
    tr = SpeakerTrainer(st, plan, Constant(1e-3, 0.9), optimizer=_sgd_cfg(), gradient_clip_val=0.05)
    head_fb = plan.head_forward_backward

    def planted(label):
        out = head_fb(label)
        st.grad[h:] = 1e6
        return out
    plan.head_forward_backward = planted
    p0 = st.flat.clone()
    tr.train_step_frozen_encoder(plan, *_batch())
    torch.cuda.synchronize()
    g = st.grad[:h].cpu()
    want, norm = _torch_sgd_step(p0[:h].cpu(), g, 0.05)
    print(f"head-only: norm hip {float(st.grad_norm[0]):.6e} torch {norm:.6e} coef {float(st.grad_norm[1]):.4f}")
    assert abs(float(st.grad_norm[0]) - float(torch.linalg.vector_norm(g.double()))) <= 1e-6 * norm
    assert float(st.grad_norm[1]) < 1.0                   # the clip engaged
    assert torch.allclose(st.flat[:h].cpu(), want, atol=1e-6, rtol=0)
    assert torch.equal(st.flat[h:], p0[h:])               # body and CNN bit-unchanged
    assert (st.step_head, st.step_body) == (1, 0)


def _tri(steps, base):
    from w2v2_speaker_amd.optim.schedule import LambdaSchedule, TriStageLearningRateLambdaLRFunction
    return LambdaSchedule(base, TriStageLearningRateLambdaLRFunction(steps, 0.2, 0.4, 0.4, base / 10, base, base / 10), 0.9)


@pytest.mark.parametrize("schedule", ["constant", "tri_stage"])
def test_fifteen_sgd_steps_reduce_the_loss(schedule):
    """Fifteen clipped Nesterov-SGD steps on the fixed batch reduce the loss, under a constant lr and under tri-stage.
    lr 2e-2 with the gradient clipped to norm 1: a step moves the parameters by at most lr * (1 + momentum) per unit
    of clipped gradient, comparable to the Adam test's 1e-3 per element."""
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    st = _store(torch.float32)
    sched = Constant(2e-2, 0.9) if schedule == "constant" else _tri(16, 2e-2)
    tr = SpeakerTrainer(st, Plan(st, 4, 4000, train=True, reg=_no_reg()), sched, optimizer=_sgd_cfg(), gradient_clip_val=1.0)
    wav, label = _batch()
    losses = [float(tr.train_step(wav, label, skip_layers=())[0]) for _ in range(16)]
    print(schedule, ["%.3f" % l for l in losses])
    assert all(np.isfinite(l) for l in losses) and losses[-1] < losses[0], losses


def test_adam_weight_decay_through_the_trainer_matches_torch():
    """Adam with L2 weight decay 1e-2 and a clip that engages, one step, against CPU torch on the device's gradient.
    The first Adam step moves an element by u(gr) = lr * gr / (|gr| + eps) with gr = g * coef + wd * p.  Where the two
    terms cancel, or both are small, |gr| comes down to eps = 1e-8 and the step is ill-conditioned:
    |du / dgr| = lr * eps / (|gr| + eps)^2, up to lr / eps = 1e5.  What gr may differ by between torch and the kernel:
    torch's coefficient comes from an f32 norm over n = 87 k elements (sqrt(n) * 2^-24 = 1.8e-5 relative, taken as
    2e-5), the kernel's from a double one; plus two f32 roundings of the terms.  So per element
        tol = 1e-6 + sens * d,   d = 2e-5 |g coef| + 2.4e-7 (|g coef| + |wd p|),
        sens = lr eps / (max(|gr| - d, 0) + eps)^2   (the largest slope within d of gr),
    and plain atol 1e-6 (the Adam test's bound) wherever |gr| > 1e-5, where sens * d < 1e-3 * 1e-8 / 1e-10 * 2e-8."""
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim import OptimConfig
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    lr, eps, wd = 1e-3, 1e-8, 1e-2
    st = _store(torch.float32)
    tr = SpeakerTrainer(st, Plan(st, 4, 4000, train=True, reg=_no_reg()), Constant(lr, 0.9),
                        optimizer=OptimConfig("adam", weight_decay=wd), gradient_clip_val=0.5)
    p0 = st.flat.clone()
    tr.train_step(*_batch(), skip_layers=())
    torch.cuda.synchronize()
    n = st.n_train
    p = torch.nn.Parameter(p0[:n].cpu().clone())
    p.grad = st.grad[:n].cpu().clone()
    torch.nn.utils.clip_grad_norm_([p], 0.5)
    gc, wp = p.grad.double().abs(), (wd * p.detach().double()).abs()
    gr = (p.grad.double() + wd * p.detach().double()).abs()
    torch.optim.Adam([p], lr=lr, weight_decay=wd, eps=eps).step()
    assert float(st.grad_norm[1]) < 1.0
    err = (st.flat[:n].cpu() - p.detach()).abs().double()
    d = 2e-5 * gc + 2.4e-7 * (gc + wp)
    tol = 1e-6 + lr * eps / ((gr - d).clamp(min=0) + eps) ** 2 * d
    well = gr > 1e-5
    print(f"adam wd+clip: max err {float(err[well].max()):.2e} where |gr| > 1e-5, {float(err[~well].max()):.2e} elsewhere "
          f"({int((~well).sum())} of {n} elements); worst err / tol {float((err / tol).max()):.3f}")
    assert float(err[well].max()) <= 1e-6
    assert bool((err <= tol).all())
    assert torch.equal(st.flat[n:], p0[n:])


def test_default_trainer_issues_the_old_launches():
    """Default arguments: the step goes through adam_step and never through the new entry points."""
    from w2v2_speaker_amd import ops
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    st = _store(torch.float16)
    tr = SpeakerTrainer(st, Plan(st, 4, 4000, train=True, reg=_no_reg()), Constant(1e-3, 0.9))
    calls = []
    orig = {n: getattr(ops, n) for n in ("adam_step", "optim_step", "grad_norm", "grad_scaler_check")}
    try:
        for n, fn in orig.items():
            setattr(ops, n, (lambda n_, fn_: lambda *a, **k: (calls.append(n_), fn_(*a, **k))[1])(n, fn))
        tr.train_step(*_batch(), skip_layers=())
        assert calls == ["grad_scaler_check", "adam_step"], calls
        del calls[:]
        tr.gradient_clip_val = 1.0           # clipping on in fp16: the norm pass replaces the found_inf scan
        tr.train_step(*_batch(), skip_layers=())
        assert calls == ["grad_norm", "optim_step"], calls
    finally:
        for n, fn in orig.items():
            setattr(ops, n, fn)


# ------------------------------------------------------------------------------------------------- ECAPA
def test_ecapa_sgd_clip_step_matches_torch():
    """One EcapaTrainer step at the smallest configuration of tests/test_ecapa_gpu.py under SGD + clip against CPU torch on
    the device's gradient.  atol 1e-6: the bound of the wav2vec2 step above (same kernel, same lr, parameters of the
    same magnitude; that file has no numeric bound of its own for an optimiser step)."""
    from w2v2_speaker_amd.ecapa import EcapaPlan, EcapaTrainer
    from w2v2_speaker_amd.optim.schedule import Constant
    import test_ecapa_gpu as TE
    cfg, ocfg, st, sd, feat, label = TE._setup(torch.float32)
    plan = EcapaPlan(st, feat.shape[0], feat.shape[1], train=True)
    tr = EcapaTrainer(st, plan, Constant(1e-3, 0.9), optimizer=_sgd_cfg(), gradient_clip_val=0.1)
    p0 = st.flat.clone()
    tr.train_step(feat.to(DEV), label.to(DEV))
    torch.cuda.synchronize()
    g = st.grad.cpu()
    want, norm = _torch_sgd_step(p0.cpu(), g, 0.1)
    print(f"ecapa: norm hip {float(st.grad_norm[0]):.6e} torch {norm:.6e} coef {float(st.grad_norm[1]):.4f}")
    assert abs(float(st.grad_norm[0]) - float(torch.linalg.vector_norm(g.double()))) <= 1e-6 * norm
    assert float(st.grad_norm[1]) < 1.0
    assert torch.allclose(st.flat.cpu(), want, atol=1e-6, rtol=0)
    assert st.exp_avg_sq is None


# ------------------------------------------------------------------------------------------------- module surface
def _module(**kw):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import Wav2vec2FCModule, Wav2vec2FCModuleConfig
    tiny = W2V2Config.tiny()
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: tiny)
    mcfg = Wav2vec2FCModuleConfig(reset_weights=True, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                                  hidden_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0)
    try:
        if "checkpoint_path" in kw:
            from w2v2_speaker_amd.optim.loss import AngularAdditiveMarginSoftMaxLoss
            ctor = lambda: AngularAdditiveMarginSoftMaxLoss(2, 2, margin=0.2, scale=30, device=DEV, act_dtype=torch.float32)
            return Wav2vec2FCModule.load_from_checkpoint(kw.pop("checkpoint_path"), cfg=mcfg, num_speakers=10,
                                                         loss_fn_constructor=ctor, device=DEV, act_dtype=torch.float32,
                                                         init_seed=99, **kw)
        return Wav2vec2FCModule.from_config(mcfg, num_speakers=10, device=DEV, act_dtype=torch.float32, init_seed=5, **kw)
    finally:
        W2V2Config.from_huggingface_id = orig


def _reference_two_lines(module, steps=20):
    """What ref: src/main.py:323-335 does with its instantiated optimiser and schedule."""
    from torch.optim.lr_scheduler import LambdaLR
    from w2v2_speaker_amd.optim.schedule import TriStageLearningRateLambdaLRFunction
    opt = torch.optim.SGD(module.parameters(), lr=3e-3, momentum=0.9, nesterov=True)
    module.set_optimizer(opt)
    module.set_lr_schedule({"scheduler": LambdaLR(opt, TriStageLearningRateLambdaLRFunction(steps, 0.1, 0.4, 0.5, 3e-4, 3e-3, 3e-5)),
                            "interval": "step"})
    return opt


def _mbatch():
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import SpeakerClassificationDataBatch
    wav, label = O.synth_batch(4, 4000, 10, seed=3)
    return SpeakerClassificationDataBatch(4, ["a", "b", "c", "d"], wav, label).to(DEV)


def test_module_set_optimizer_and_schedule_drive_the_fused_step():
    from w2v2_speaker_amd.optim import OptimConfig
    from w2v2_speaker_amd.optim.schedule import LambdaSchedule, TriStageLearningRateLambdaLRFunction
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    mod = _module(gradient_clip_val=0.5)
    assert mod.configure_optimizers() is None
    opt = _reference_two_lines(mod)
    got = mod.configure_optimizers()
    assert got[0] == [opt] and got[1][0]["interval"] == "step"
    assert mod.optimizer_cfg == OptimConfig("sgd", momentum=0.9, nesterov=True)
    batch = _mbatch()
    mod.train()
    mod.on_train_start()
    p0 = mod.store.flat.clone()
    for i in range(2):
        mod.training_step(batch, i)
    torch.cuda.synchronize()
    # the same two steps at trainer level on a twin store
    twin = _module()
    assert torch.equal(twin.store.flat, p0)
    sched = LambdaSchedule(3e-3, TriStageLearningRateLambdaLRFunction(20, 0.1, 0.4, 0.5, 3e-4, 3e-3, 3e-5), 0.9)
    tr = SpeakerTrainer(twin.store, twin._plan(4, 4000, True), sched, optimizer=OptimConfig("sgd", momentum=0.9, nesterov=True),
                        gradient_clip_val=0.5)
    for i in range(2):
        tr.train_step(batch.network_input[:, 0], batch.ground_truth)
    torch.cuda.synchronize()
    assert not torch.equal(mod.store.flat, p0)
    assert torch.equal(mod.store.flat, twin.store.flat)
    assert float(mod.store.grad_norm[1]) < 1.0
    with pytest.raises(NotImplementedError, match="AdamW"):
        mod.set_optimizer(torch.optim.AdamW(mod.parameters(), lr=1e-3))
    with pytest.raises(NotImplementedError, match="interval"):
        mod.set_lr_schedule({"scheduler": got[1][0]["scheduler"], "interval": "epoch"})


def test_sgd_checkpoint_loads_into_torch_and_resumes_bit_for_bit(tmp_path):
    """optimizer_states[0] of a file saved under SGD is a torch.optim.SGD.state_dict() over module.parameters();
    save -> load -> step == the uninterrupted run, bit for bit; a file written under SGD does not load under Adam."""
    batch = _mbatch()
    a = _module(gradient_clip_val=0.5)
    _reference_two_lines(a)
    a.train()
    a.on_train_start()
    for i in range(2):
        a.training_step(batch, i)
    path = str(tmp_path / "sgd.ckpt")
    a.save_checkpoint(path)
    a.training_step(batch, 2)
    torch.cuda.synchronize()
    ck = torch.load(path, weights_only=False)
    osd = ck["optimizer_states"][0]
    group = osd["param_groups"][0]
    assert group["momentum"] == 0.9 and group["nesterov"] is True and group["dampening"] == 0 and group["weight_decay"] == 0
    assert "betas" not in group and ck["lr_schedulers"][0]["last_epoch"] == 2
    b = _module(checkpoint_path=path, gradient_clip_val=0.5)
    opt = _reference_two_lines(b)
    opt.load_state_dict(osd)                                  # what PL's restore does with it
    params = list(b.parameters())
    names = b.store.reference_parameter_order()
    for i, (n, p) in enumerate(zip(names, params)):
        if b.store.is_trainable(n):
            assert tuple(opt.state[p]["momentum_buffer"].shape) == tuple(p.shape), n
        else:
            assert p not in opt.state
    b._torch_schedule["scheduler"].load_state_dict(ck["lr_schedulers"][0])
    assert b._torch_schedule["scheduler"].last_epoch == 2
    b.train()
    b.training_step(batch, 2)
    torch.cuda.synchronize()
    assert b.schedule_step == a.schedule_step == 3
    assert torch.equal(b.store.flat, a.store.flat) and torch.equal(b.store.exp_avg, a.store.exp_avg)
    # the other algorithm refuses the state
    c = _module()
    c.train()
    c.training_step(batch, 0)                                 # default Adam: the arenas now hold Adam moments
    with pytest.raises(RuntimeError, match="adam"):
        c.store.load_torch_optimizer_state(osd)
    d = _module(checkpoint_path=path)
    d.set_optimizer(torch.optim.Adam(d.parameters(), lr=1e-3))
    d.train()
    with pytest.raises(RuntimeError, match="sgd"):
        d.training_step(batch, 0)


def test_ecapa_and_paired_modules_take_the_reference_optimizer_and_schedule():
    """The same two calls on EcapaTdnnModule and Wav2vec2PairedSpeakerModule (the smallest configurations of
    tests/test_surface_gpu.py): SGD under OneCycleLR (momentum cycled) resp. Adam with weight decay under tri-stage,
    with clipping; a few steps through the public surface lower the loss, the state arenas are the algorithm's, and
    the norm record is live."""
    from torch.optim.lr_scheduler import LambdaLR, OneCycleLR
    from w2v2_speaker_amd import config as C
    from w2v2_speaker_amd.lightning_modules.speaker.ecapa_tdnn import EcapaTDNNModuleConfig, EcapaTdnnModule
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import SpeakerClassificationDataBatch
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_paired_input import (
        PairedSpeakerClassificationDataBatch, Wav2vec2PairedSpeakerModule, Wav2vec2PairedSpeakerModuleConfig)
    from w2v2_speaker_amd.optim import OptimConfig
    from w2v2_speaker_amd.optim.loss import AngularAdditiveMarginSoftMaxLoss, BinaryCrossEntropyLoss
    from w2v2_speaker_amd.optim.schedule import LambdaSchedule, OneCycle, TriStageLearningRateLambdaLRFunction
    g = torch.Generator().manual_seed(0)
    ecfg = EcapaTDNNModuleConfig(input_mel_coefficients=16, lin_neurons=24, channels=[64, 64, 64, 64, 192],
                                 attention_channels=16, res2net_scale=4, se_channels=16)
    actor = lambda: AngularAdditiveMarginSoftMaxLoss(2, 2, margin=0.2, scale=30.0, device=DEV, act_dtype=torch.float32)
    em = EcapaTdnnModule(None, ecfg, 5, actor, [], [], None, gradient_clip_val=1.0)
    opt = torch.optim.SGD(em.parameters(), lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)
    em.set_optimizer(opt)
    em.set_lr_schedule({"scheduler": OneCycleLR(opt, max_lr=2e-2, total_steps=50), "interval": "step"})
    assert em.optimizer_cfg.algo == "sgd" and em.optimizer_cfg.nesterov and isinstance(em.schedule, OneCycle)
    assert em.configure_optimizers()[0] == [opt]
    feat = torch.randn(6, 40, 16, generator=g)
    batch = SpeakerClassificationDataBatch(6, [str(i) for i in range(6)], feat, torch.randint(0, 5, (6,), generator=g))
    losses = [float(em.training_step(batch)["loss"]) for _ in range(12)]
    print("ecapa module, SGD + one-cycle + clip:", ["%.3f" % l for l in losses], em.store.grad_norm.tolist())
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert em.store.optim_algo == "sgd" and em.store.exp_avg is not None and em.store.exp_avg_sq is None
    assert float(em.store.grad_norm[0]) > 0 and 0 < float(em.store.grad_norm[1]) <= 1.0
    tiny = C.W2V2Config.tiny()
    orig = C.W2V2Config.from_huggingface_id
    C.W2V2Config.from_huggingface_id = staticmethod(lambda _id: tiny)
    try:
        pm = Wav2vec2PairedSpeakerModule(None, Wav2vec2PairedSpeakerModuleConfig(), BinaryCrossEntropyLoss, gradient_clip_val=1.0)
    finally:
        C.W2V2Config.from_huggingface_id = orig
    pm.store.scaler[0] = 256.0
    opt = torch.optim.Adam(pm.parameters(), lr=2e-3, weight_decay=1e-3)
    pm.set_optimizer(opt)
    pm.set_lr_schedule(LambdaLR(opt, TriStageLearningRateLambdaLRFunction(50, 0.1, 0.4, 0.5, 2e-4, 2e-3, 2e-5)))
    assert pm.optimizer_cfg == OptimConfig("adam", weight_decay=1e-3) and isinstance(pm.schedule, LambdaSchedule)
    a, b = 0.3 * torch.randn(4, 4000, generator=g), 0.3 * torch.randn(4, 4000, generator=g)
    pb = PairedSpeakerClassificationDataBatch(4, list("abcd"), a, list("efgh"), b, torch.tensor([1, 0, 1, 0]))
    pl = [float(pm.training_step(pb)["loss"]) for _ in range(10)]
    print("paired module, Adam + weight decay + tri-stage + clip:", ["%.3f" % l for l in pl], pm.store.grad_norm.tolist())
    assert np.isfinite(pl).all() and pl[-1] < pl[0]
    assert float(pm.store.scaler[3]) == 0.0 and float(pm.store.grad_norm[0]) > 0
