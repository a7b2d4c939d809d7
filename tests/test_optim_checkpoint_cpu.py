"""The optimiser half of a checkpoint under SGD / weight decay / tri-stage, on the host: the emitted
``optimizer_states[0]`` and ``lr_schedulers[0]`` go into REAL torch objects, and a state written under one algorithm is
refused under the other.  (The stepped, bit-for-bit resume runs on the GPU: tests/test_optim_trainer_gpu.py.)"""
import copy

import pytest
import torch


def _module(**kw):
    from w2v2_speaker_amd import config as C
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import Wav2vec2FCModule, Wav2vec2FCModuleConfig
    tiny = C.W2V2Config.tiny()
    orig = C.W2V2Config.from_huggingface_id
    C.W2V2Config.from_huggingface_id = staticmethod(lambda _id: tiny)       # keep the CPU test small
    try:
        return Wav2vec2FCModule.from_config(Wav2vec2FCModuleConfig(reset_weights=True), num_speakers=7, init_seed=1,
                                            device="cpu", act_dtype=torch.float32, **kw)
    finally:
        C.W2V2Config.from_huggingface_id = orig


def _pretend_steps(store, algo, steps=4):
    """What `steps` optimiser steps leave behind on the host side (no kernels on this machine)."""
    g = torch.Generator().manual_seed(7)
    store.optim_algo = algo
    store.exp_avg = torch.randn(store.n_train, generator=g)
    if algo == "adam":
        store.exp_avg_sq = torch.rand(store.n_train, generator=g)
    store.set_step_counts(steps, steps)


def test_sgd_tri_stage_checkpoint_feeds_torch_sgd_and_lambda_lr(tmp_path):
    from torch.optim.lr_scheduler import LambdaLR
    from w2v2_speaker_amd.optim.schedule import TriStageLearningRateLambdaLRFunction as Tri
    a = _module()
    tri = dict(max_steps=100, warmup_stage_ratio=0.1, constant_stage_ratio=0.4, decay_stage_ratio=0.5, initial_lr=3e-4,
               base_lr=3e-3, final_lr=3e-5)
    opt = torch.optim.SGD(a.parameters(), lr=3e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)
    a.set_optimizer(opt)
    a.set_lr_schedule({"scheduler": LambdaLR(opt, Tri(**tri)), "interval": "step"})
    assert a.configure_optimizers()[0] == [opt]
    _pretend_steps(a.store, "sgd")
    a.steps = a.schedule_step = 4
    path = str(tmp_path / "sgd.ckpt")
    a.save_checkpoint(path)
    ck = torch.load(path, weights_only=False)
    osd, ssd = ck["optimizer_states"][0], ck["lr_schedulers"][0]
    group = osd["param_groups"][0]
    assert group["weight_decay"] == 1e-4 and group["momentum"] == 0.9 and group["nesterov"] is True and group["dampening"] == 0
    assert group["lr"] == pytest.approx(3e-3 * Tri(**tri)(4)) and group["initial_lr"] == 3e-3
    # a fresh torch optimiser + scheduler over a fresh module's parameters take both, and step
    b = _module()
    params = list(b.parameters())
    opt2 = torch.optim.SGD(params, lr=3e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)
    sch2 = LambdaLR(opt2, Tri(**tri))
    opt2.load_state_dict(copy.deepcopy(osd))             # (torch adopts the tensors it is given; step() below writes them)
    sch2.load_state_dict(ssd)
    names = b.store.reference_parameter_order()
    for n, p in zip(names, params):
        if b.store.is_trainable(n):
            assert torch.equal(opt2.state[p]["momentum_buffer"], a.store._view(a.store.exp_avg, n)), n
        else:
            assert p not in opt2.state
    for p in params:
        p.grad = torch.zeros_like(p) if p.grad is None else p.grad
    opt2.step()
    sch2.step()
    assert sch2.last_epoch == 5 and opt2.param_groups[0]["lr"] == pytest.approx(3e-3 * Tri(**tri)(5))
    # the store takes it back, and refuses it under the other algorithm
    b.store.load_torch_optimizer_state(osd)
    assert b.store.optim_algo == "sgd" and b.store.exp_avg_sq is None
    assert all(torch.equal(b.store._view(b.store.exp_avg, n), a.store._view(a.store.exp_avg, n))
               for n in names if b.store.is_trainable(n))
    c = _module()
    _pretend_steps(c.store, "adam")
    with pytest.raises(RuntimeError, match="adam"):
        c.store.load_torch_optimizer_state(osd)
    with pytest.raises(RuntimeError, match="sgd"):
        b.store.torch_adam_state(1e-3)


def test_adam_checkpoint_carries_the_real_weight_decay(tmp_path):
    a = _module()
    a.set_optimizer(torch.optim.Adam(a.parameters(), lr=1e-4, weight_decay=1e-3))
    _pretend_steps(a.store, "adam")
    path = str(tmp_path / "adam.ckpt")
    a.save_checkpoint(path)
    osd = torch.load(path, weights_only=False)["optimizer_states"][0]
    assert osd["param_groups"][0]["weight_decay"] == 1e-3 and "betas" in osd["param_groups"][0]
    assert a.store.torch_adam_state(1e-3)["param_groups"][0]["weight_decay"] == 0        # the old name: plain Adam
    opt = torch.optim.Adam(list(_module().parameters()), lr=1e-4, weight_decay=1e-3)
    opt.load_state_dict(osd)
    b = _module()
    b.store.load_torch_adam_state(osd)                     # (alias of load_torch_optimizer_state)
    assert b.store.optim_algo == "adam" and (b.store.step_head, b.store.step_body) == (4, 4)
