"""wav2spk on the CPU: the float64 restatement of tests/wav2spk_cases.py against the golden of the reference's layer list,
the parameter table, the frame formula, the MultiStep schedule, the error branches and the state-dict round trip.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import wav2spk_cases as K
from w2v2_speaker_amd import wav2spk as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    meta = json.load(open(os.path.join(GOLDEN, "g23_wav2spk.json")))
    return meta, np.load(os.path.join(GOLDEN, "g23_wav2spk.npz"))


def _rel(got, ref):
    got, ref = torch.as_tensor(np.asarray(got), dtype=K.F64), torch.as_tensor(np.asarray(ref), dtype=K.F64)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300)) if float(ref.norm()) > 0 else float((got - ref).norm())


@pytest.mark.parametrize("case", range(len(K.STEP_CASES) * len(K.GATINGS) * len(K.POOLINGS)))
def test_float64_restatement_reproduces_the_golden(golden, case):
    meta, g = golden
    c = meta["cases"][case]
    tag, gating, pooling = c["tag"], c["gating"], c["pooling"]
    wav, label = K.synth_batch(c["batch"], c["samples"])
    sd = K.make_state_dict(pooling=pooling)
    rec = K.forward_ref(sd, wav, label, gating, pooling)
    worst = abs(float(rec["loss"]) - float(g[f"{tag}.loss"])) / float(g[f"{tag}.loss"])
    assert list(rec["stage"]) == K.stage_names(gating)
    for n, t in rec["stage"].items():
        worst = max(worst, abs(float(t.norm()) / float(g[f"{tag}.stage.{n}.norm"]) - 1), _rel(K.strided(t), g[f"{tag}.stage.{n}.sample"]))
    for i in K.EMBEDDING_LAYERS:
        worst = max(worst, _rel(K.strided(K.embedding_of(rec, i), 1024), g[f"{tag}.emb.{i}"]))
    grads = K.backward_ref(sd, rec)
    assert list(grads) != [] and set(grads) == set(sd)
    for n, gr in grads.items():
        if n.startswith("encoder.") and n.endswith("bias"):
            # the reference's autograd leaves rounding noise here (1e-16 .. 1e-19 in float64); the restatement has exact zeros
            assert float(gr.abs().max()) == 0.0 and float(np.abs(g[f"{tag}.grad.{n}"]).max()) < 1e-12
            continue
        if gr.numel() <= 512:
            worst = max(worst, _rel(gr, g[f"{tag}.grad.{n}"]))
        else:
            ref_norm = float(g[f"{tag}.grad.{n}.norm"])
            if ref_norm == 0.0:                                   # the gate's parameters when it is not applied
                assert float(gr.norm()) == 0.0
                continue
            worst = max(worst, abs(float(gr.norm()) / ref_norm - 1), _rel(K.strided(gr), g[f"{tag}.grad.{n}.sample"]))
    print(f"{tag}: worst relative difference to the golden {worst:.2e}")
    assert worst <= TOL


def test_parameter_names_shapes_and_count():
    cfg = W.Wav2SpkConfig()
    shapes = W.wav2spk_param_shapes(cfg, K.SPEAKERS)
    assert list(shapes.items()) == list(K.param_shapes().items())
    assert sum(int(np.prod(s)) for s in shapes.values()) == K.PARAMETERS == 5590995
    mean = W.wav2spk_param_shapes(W.Wav2SpkConfig(stat_pooling_type="mean", hidden_fc_layers_out=()), 11)
    assert mean["fc_list.0.0.weight"] == (11, 512) and "fc_list.1.0.weight" not in mean
    assert cfg.embedding_size(7) == 512 and W.Wav2SpkConfig(embedding_layer_idx=-1).embedding_size(7) == 1024
    assert W.Wav2SpkConfig(embedding_layer_idx=2).embedding_size(7) == 7
    with pytest.raises(ValueError):
        W.Wav2SpkConfig(embedding_layer_idx=3)
    with pytest.raises(ValueError):
        W.Wav2SpkConfig(stat_pooling_type="max")


def test_frame_formula_matches_torch_conv1d():
    assert W.wav2spk_frames(3200) == (640, 160, 80, 40, 20) and W.wav2spk_frames(805) == (161, 41, 21, 11, 6)
    for n in range(160, 2001):
        x, got = torch.zeros(1, 1, n), []
        for cin, cout, k, s, p in W.ENCODER:
            x = torch.nn.functional.conv1d(x[:, :1], torch.zeros(1, 1, k), stride=s, padding=p)
            got.append(x.shape[2])
        assert W.wav2spk_frames(n) == tuple(got), n
    lo = W.wav2spk_min_samples()
    assert min(W.wav2spk_frames(lo)) == W.MIN_FRAMES and min(W.wav2spk_frames(lo - 1)) < W.MIN_FRAMES


def test_multistep_schedule_matches_torch_step_by_step():
    from w2v2_speaker_amd.optim.schedule import MultiStep, from_torch_scheduler
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[3, 7, 7, 12, 20], gamma=0.1)
    ours = from_torch_scheduler(sched)
    assert isinstance(ours, MultiStep) and ours.gamma == 0.1 and list(ours.milestones) == [3, 7, 7, 12, 20]
    for step in range(26):
        lr, beta1 = ours.at(step)
        assert lr == opt.param_groups[0]["lr"] and beta1 == 0.9, step
        opt.step()
        sched.step()
    assert MultiStep(1e-3, [300_000, 450_000], 0.1).at(449_999)[0] == pytest.approx(1e-4, rel=1e-15)
    with pytest.raises(NotImplementedError, match="StepLR"):
        from_torch_scheduler(torch.optim.lr_scheduler.StepLR(opt, 10))


def test_error_branches():
    from w2v2_speaker_amd.lightning_modules.speaker import Wav2SpkModule, Wav2SpkModuleConfig
    from w2v2_speaker_amd.optim.loss import AngularAdditiveMarginSoftMaxLoss
    with pytest.raises(NotImplementedError):
        W.Wav2SpkStore(W.Wav2SpkConfig(), "cpu", torch.bfloat16, num_speakers=7)
    aam = lambda: AngularAdditiveMarginSoftMaxLoss(2, 2, margin=0.2, scale=30.0, device="cpu", act_dtype=torch.float32)
    with pytest.raises(ValueError, match="wav2spk does not support aam softmax"):
        Wav2SpkModule(None, Wav2SpkModuleConfig(), 7, aam, device="cpu")
    with pytest.raises(NotImplementedError):
        Wav2SpkModule(None, Wav2SpkModuleConfig(), 7, lambda: object(), device="cpu")
    with pytest.raises(NotImplementedError):
        Wav2SpkModule.from_config(Wav2SpkModuleConfig(), 7, device="cpu", act_dtype=torch.bfloat16)
    st = W.Wav2SpkStore(W.Wav2SpkConfig(), "cpu", num_speakers=7)
    with pytest.raises(ValueError, match="samples"):
        W.Wav2SpkPlan(st, 1, W.wav2spk_min_samples() - 1, train=False)                 # too short
    with pytest.raises(ValueError):
        W.valid_sample_lengths([805, 100], 2, 3200)
    with pytest.raises(ValueError):
        W.valid_sample_lengths([805, 3201], 2, 3200)
    with pytest.raises(ValueError):
        W.valid_sample_lengths([805], 2, 3200)
    assert W.valid_sample_lengths(torch.tensor([805, 3200]), 2, 3200) == [805, 3200]


def test_state_dict_round_trip_and_init():
    cfg = W.Wav2SpkConfig()
    a, b = W.Wav2SpkStore(cfg, "cpu", num_speakers=7), W.Wav2SpkStore(cfg, "cpu", num_speakers=7)
    a.init_weights(5)
    sd = a.state_dict()
    assert list(sd) == list(K.param_shapes()) and all(tuple(v.shape) == K.param_shapes()[n] for n, v in sd.items())
    assert float(sd["encoder.0.0.bias"].abs().max()) > 0 and float(sd["encoder.0.0.weight"].abs().max()) <= 10 ** -0.5
    assert abs(float(sd["temporal_gate.W"].std()) - (2 / 1024) ** 0.5) < 2e-3
    b.load_state_dict(sd)
    assert torch.equal(a.flat, b.flat)
    del sd["temporal_gate.b"]
    with pytest.raises(KeyError):
        b.load_state_dict(sd)
