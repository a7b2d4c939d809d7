"""The wav2spk path on the device (w2v2_speaker_amd/wav2spk.py, csrc/wav2spk.hip): every new kernel against float64 of its
stored operands, two whole training steps stage by stage and gradient by gradient against the float64 restatement of
tests/wav2spk_cases.py, the evaluation contract (a row of a padded batch is the utterance alone, bit for bit) and the module.

Bounds.  A stage is f32 from stored f32 operands: 2e-5 rel-L2, the project's f32 stage bound (F32_BOUND); sums whose terms
cancel (dW of layer 0, bias gradients, the two means of the InstanceNorm backward) are held to 2e-5 of the sum of their
|terms|.  The end-to-end error of the 14-stage f32 chain cannot be derived, so the whole-step tests measure it on the
reference's own arithmetic: the same stack in torch f32 on the CPU against float64 gives E_ref (the largest rel-L2 error over
all weight gradients of the case) and E_stage (over all stage outputs); the device is held to twice those -- the factor 2
covers a different summation order, nothing more.  The worst figure per kind is printed before anything is asserted
(``pytest -s``; profiles/wav2spk_parity.txt)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import wav2spk_cases as K
from w2v2_speaker_amd import ops
from w2v2_speaker_amd import wav2spk as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
BOUND = K.F32_BOUND
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class _Report:
    """Worst figure per stage kind (printed before anything is asserted) and the list of misses."""

    def __init__(self, tag: str, bound: float = BOUND):
        self.tag, self.bound, self.worst, self.bad = tag, bound, {}, []

    def note(self, kind, item, err, bound=None):
        bound = self.bound if bound is None else bound
        if kind not in self.worst or err > self.worst[kind][0] or err != err:
            self.worst[kind] = (err, item, bound)
        if not err <= bound:
            self.bad.append((kind, item, err, bound))

    def stage(self, kind, item, got, ref, bound=None):
        assert got.shape == ref.shape, (kind, item, got.shape, ref.shape)
        self.note(kind, item, K.rel_l2(got, ref), bound)

    def sums(self, kind, item, got, ref, sum_abs):
        assert got.shape == ref.shape == sum_abs.shape, (kind, item)
        self.note(kind + " /sum|terms|", item, K.sum_scale_error(got, ref, sum_abs))

    def flush(self):
        for kind, (err, item, bound) in self.worst.items():
            print(f"wav2spk-parity: {self.tag} {kind}: worst {err:.2e} bound {bound:.2e} ({item})")
        assert not self.bad, (self.tag, self.bad[:6], len(self.bad))


def _cpu(t):
    return None if t is None else t.detach().cpu()


def _lens(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ layer 0
@pytest.mark.parametrize("N", K.FIRST_SAMPLES)
def test_conv1d_first_forward_backward_and_lengths_vs_float64(N):
    k, s, p = K.FIRST
    rep = _Report(f"conv1d_first N={N}")
    for C in (40, 44):
        g = torch.Generator().manual_seed(N + C)
        B, T = 3, K.frames_of(N, k, s, p)
        wav, w, b = torch.randn(B, N, generator=g), torch.randn(C, 1, k, generator=g) * 0.3, torch.randn(C, generator=g)
        z = torch.full((B * T, C), float("nan"), device=DEV)
        ops.conv1d_first(wav.to(DEV), w.to(DEV), b.to(DEV), z, C, k, s, p)
        rep.stage("z", f"C={C}", _cpu(z).view(B, T, C), K.first_fwd_ref(wav, w, b))
        # the weight gradient: a sum over all B * T rows whose terms cancel
        dz = torch.randn(B * T, C, generator=g)
        dw = torch.zeros(C, 1, k, device=DEV)
        work = ops.conv1d_first_bwd_workspace(B * T, C, k, DEV)
        ops.conv1d_first_bwd(wav.to(DEV), dz.to(DEV), C, work, dw, k, s, p)
        dW, _, _, dW_abs = K.conv_bwd_ref(wav.reshape(B * N, 1), w, dz, B, N, s, p)
        rep.sums("dW", f"C={C}", _cpu(dw), dW, dW_abs)
        rep.stage("dW", f"C={C}", _cpu(dw), dW)
        dw2 = torch.zeros(C, 1, k, device=DEV)
        ops.conv1d_first_bwd(wav.to(DEV), dz.to(DEV), C, work, dw2, k, s, p)
        assert torch.equal(dw, dw2)                                              # fixed order: bitwise reproducible
        # lengths: samples past n_b count as zero (here they hold junk), rows past the utterance's frames are zeros
        lens = [N, max(K.FIRST_SAMPLES[0], N - 3), K.FIRST_SAMPLES[0]]
        junk = wav.clone()
        for i, n in enumerate(lens):
            junk[i, n:] = 1e3
        zl = torch.full((B * T, C), float("nan"), device=DEV)
        ops.conv1d_first(junk.to(DEV), w.to(DEV), b.to(DEV), zl, C, k, s, p, lens=_lens(lens))
        rep.stage("z (lens)", f"C={C}", _cpu(zl).view(B, T, C), K.first_fwd_ref(wav, w, b, lens))
        for i, n in enumerate(lens):
            Tn = K.frames_of(n, k, s, p)
            alone = torch.empty(Tn, C, device=DEV)
            ops.conv1d_first(wav[i:i + 1, :n].contiguous().to(DEV), w.to(DEV), b.to(DEV), alone, C, k, s, p)
            assert torch.equal(zl.view(B, T, C)[i, :Tn], alone) and not bool(zl.view(B, T, C)[i, Tn:].any()), (C, i, n)
    rep.flush()


# ------------------------------------------------------------------------------------------------ gather and adjoint
@pytest.mark.parametrize("geom", K.GATHERS)
def test_im2col_zero_and_col2im_zero_vs_float64_and_adjoint_identity(geom):
    k, s, p, Tin = geom
    rep = _Report(f"gather k={k} s={s} p={p} Lin={Tin}")
    for C in K.CHANNELS:
        g = torch.Generator().manual_seed(Tin + 10 * C + k)
        B, Tout, ld = 2, K.frames_of(Tin, k, s, p), C + 4
        x = torch.randn(B * Tin, ld, generator=g)
        col = torch.full((B * Tout, k * C), float("nan"), device=DEV)
        ops.im2col_zero(x.to(DEV), ld, col, B, Tin, C, k, s, p)
        ref = K.im2col_zero_ref(x[:, :C].reshape(B, Tin, C), k, s, p)
        assert torch.equal(_cpu(col), ref.float()), C                              # a gather: exact
        d = torch.randn(B * Tout, k * C, generator=g)
        dx = torch.full((B * Tin, ld), float("nan"), device=DEV)
        ops.col2im_zero(d.to(DEV), dx, ld, B, Tin, C, k, s, p)
        got = _cpu(dx)[:, :C].reshape(B, Tin, C)
        assert bool(torch.isnan(_cpu(dx)[:, C:]).all())                           # nothing is written past the C channels
        rep.stage("col2im dx", f"C={C}", got, K.col2im_zero_ref(d, B, Tin, C, k, s, p))
        # <im2col(x), d> = <x, col2im(d)> in float64 of the two outputs
        lhs = (_cpu(col).double() * d.double()).sum()
        rhs = (x[:, :C].reshape(B, Tin, C).double() * got.double()).sum()
        scale = (_cpu(col).double() * d.double()).abs().sum()
        rep.note("adjoint identity /sum|terms|", f"C={C}", float((lhs - rhs).abs() / scale))
    rep.flush()


# ------------------------------------------------------------------------------------------------ InstanceNorm + ReLU
def _instnorm_input(B, T, C, kind):
    g = torch.Generator().manual_seed(100 * T + C)
    z = torch.randn(B, T, C, generator=g) * 1.5 + 0.3
    if kind == "dc":                  # mean / std = 300: E[z^2] - mean^2 loses five of f32's seven digits
        z = 0.01 * torch.randn(B, T, C, generator=g) + 3.0
    if kind == "constant":
        z[:, :, 5] = 0.37
        z[0, :, 9] = 0.0
    return z, torch.randn(B, T, C, generator=g)


@pytest.mark.parametrize("kind", ["plain", "dc", "constant"])
@pytest.mark.parametrize("T", K.FRAMES)
def test_instnorm_relu_kernels_vs_float64(T, kind):
    rep = _Report(f"instnorm {kind} T={T}")
    for C in K.CHANNELS:
        B = 3
        z, dy = _instnorm_input(B, T, C, kind)
        zd = z.to(DEV).view(B * T, C)
        y = torch.full((B * T, C), float("nan"), device=DEV)
        mr = torch.empty(B, C, 2, device=DEV)
        work = ops.instnorm_workspace(B, T, C, DEV)
        ops.instnorm_relu_fwd(zd, C, work, mr, y, C, B, T, C)
        f = K.instnorm_relu_ref(z)
        item = f"C={C}"
        rep.stage("mean", item, _cpu(mr)[..., 0], f["mean"])
        rep.stage("rstd", item, _cpu(mr)[..., 1], f["rstd"])
        rep.stage("var + eps = rstd^-2", item, _cpu(mr)[..., 1].double() ** -2, f["var"] + K.IN_EPS)
        rep.stage("y", item, _cpu(y).view(B, T, C), f["y"])
        if kind == "constant":
            assert not bool(_cpu(y).view(B, T, C)[:, :, 5].any()) and not bool(_cpu(y).view(B, T, C)[0, :, 9].any())
            assert K.rel_l2(_cpu(mr)[:, 5, 1], torch.full((B,), K.IN_EPS ** -0.5, dtype=F64)) <= BOUND
        assert bool((_cpu(y) == 0).any())                                           # exact zeros for the ReLU mask
        # backward from the stored z, y and statistics
        dz = torch.full((B * T, C), float("nan"), device=DEV)
        ops.instnorm_relu_bwd(dy.to(DEV).view(B * T, C), C, zd, C, y, C, mr, work, dz, C, B, T, C)
        o = K.instnorm_relu_bwd_ref(z, _cpu(y).view(B, T, C), dy, stats=_cpu(mr))
        assert bool(torch.isfinite(_cpu(dz)).all())
        rep.stage("dz", item, _cpu(dz).view(B, T, C), o["dz"])
        nblk = -(-T // 128)
        part = _cpu(work)[:B * nblk * C * 2].view(B, nblk, C, 2).double().sum(1) / T
        rep.sums("mean_t g", item, part[..., 0], o["m1"], o["m1_abs"])
        rep.sums("mean_t g zhat", item, part[..., 1], o["m2"], o["m2_abs"])
        if kind == "plain" and T >= 127:
            # (also against float64's own statistics; not at T = 2, where zhat = +-1, the three terms of dz cancel to
            # eps / var of their size and the comparison measures the f32 rounding of rstd times var / eps, not the kernel)
            rep.stage("dz (float64 chain)", item, _cpu(dz).view(B, T, C), K.instnorm_relu_bwd_ref(z, f["y"], dy)["dz"])
        # lengths: statistics over each utterance's own frames, zero rows past them, bit-identical to the utterance alone
        lens = [T, max(2, T - 1), 2]
        yl, mrl = torch.full((B * T, C), float("nan"), device=DEV), torch.empty(B, C, 2, device=DEV)
        ops.instnorm_relu_fwd(zd, C, work, mrl, yl, C, B, T, C, lens=_lens(lens))
        rep.stage("y (lens)", item, _cpu(yl).view(B, T, C), K.instnorm_relu_ref(z, lens)["y"])
        for i, n in enumerate(lens):
            ya, ma = torch.empty(n, C, device=DEV), torch.empty(1, C, 2, device=DEV)
            ops.instnorm_relu_fwd(z[i, :n].contiguous().to(DEV), C, ops.instnorm_workspace(1, n, C, DEV), ma, ya, C, 1, n, C)
            assert torch.equal(yl.view(B, T, C)[i, :n], ya) and torch.equal(mrl[i:i + 1], ma), (C, i, n)
            assert not bool(yl.view(B, T, C)[i, n:].any())
    rep.flush()


def test_instnorm_row_strides_and_reproducibility():
    B, T, C, ld = 2, 129, 44, 48
    g = torch.Generator().manual_seed(3)
    z, dy = torch.randn(B * T, ld, generator=g), torch.randn(B * T, ld, generator=g)
    y, dz = torch.full((B * T, ld), float("nan"), device=DEV), torch.full((B * T, ld), float("nan"), device=DEV)
    mr, work = torch.empty(B, C, 2, device=DEV), ops.instnorm_workspace(B, T, C, DEV)
    ops.instnorm_relu_fwd(z.to(DEV), ld, work, mr, y, ld, B, T, C)
    ops.instnorm_relu_bwd(dy.to(DEV), ld, z.to(DEV), ld, y, ld, mr, work, dz, ld, B, T, C)
    f = K.instnorm_relu_ref(z[:, :C].reshape(B, T, C))
    assert K.rel_l2(_cpu(y)[:, :C].reshape(B, T, C), f["y"]) <= BOUND
    o = K.instnorm_relu_bwd_ref(z[:, :C].reshape(B, T, C), _cpu(y)[:, :C].reshape(B, T, C), dy[:, :C].reshape(B, T, C), stats=_cpu(mr))
    assert K.rel_l2(_cpu(dz)[:, :C].reshape(B, T, C), o["dz"]) <= BOUND
    assert bool(torch.isnan(_cpu(y)[:, C:]).all()) and bool(torch.isnan(_cpu(dz)[:, C:]).all())
    y2, dz2 = torch.empty_like(y), torch.empty_like(dz)
    ops.instnorm_relu_fwd(z.to(DEV), ld, work, mr, y2, ld, B, T, C)
    ops.instnorm_relu_bwd(dy.to(DEV), ld, z.to(DEV), ld, y2, ld, mr, work, dz2, ld, B, T, C)
    assert torch.equal(y[:, :C], y2[:, :C]) and torch.equal(dz[:, :C], dz2[:, :C])
    with pytest.raises(RuntimeError, match="instnorm_relu_fwd"):
        ops.instnorm_relu_fwd(z.to(DEV), ld, work, torch.empty(B, 42, 2, device=DEV), y, ld, B, T, 42)      # C % 4 != 0


# ------------------------------------------------------------------------------------------------ gate, row ReLU
def test_gate_and_sum_bias_act_rows_vs_float64():
    rep = _Report("gate / sum_bias_act_rows")
    g = torch.Generator().manual_seed(11)
    M, Fd = 37, 44
    P, x, dy = torch.randn(M, Fd, generator=g) * 3, torch.randn(M, Fd, generator=g), torch.randn(M, Fd, generator=g)
    y, dP, dx = (torch.empty(M, Fd, device=DEV) for _ in range(3))
    ops.gate_fwd(P.to(DEV), x.to(DEV), y)
    ops.gate_bwd(dy.to(DEV), P.to(DEV), x.to(DEV), dP, dx)
    s = torch.sigmoid(P.double())
    rep.stage("gate y", "", _cpu(y), s * x.double())
    rep.stage("gate dP", "", _cpu(dP), dy.double() * x.double() * s * (1 - s))
    rep.stage("gate dx (direct)", "", _cpu(dx), dy.double() * s)
    B, T, C, lens = 3, 9, 44, [9, 4, 2]
    own = (torch.arange(T)[None] < torch.tensor(lens)[:, None])[..., None]
    for S in (1, 3):
        parts, bias = torch.randn(S, B * T, C, generator=g), torch.randn(C, generator=g)
        total = parts.double().sum(0)
        for relu in (False, True):
            act = (lambda v: v.clamp_min(0)) if relu else (lambda v: v)
            r = torch.full((B * T, C), float("nan"), device=DEV)
            ops.sum_bias_act_rows(parts.to(DEV), bias.to(DEV), r, B, T, C, relu)
            rep.stage("sum + bias" + (" + relu" if relu else ""), f"S={S}", _cpu(r), act(total + bias.double()))
            pd = parts.to(DEV)
            ops.sum_bias_act_rows(pd, None, pd[0], B, T, C, relu, lens=_lens(lens))       # no bias, in place on the first part
            rep.stage("sum (lens)" + (" + relu" if relu else ""), f"S={S}", _cpu(pd[0]).view(B, T, C), act(total).view(B, T, C) * own)
            assert not bool((_cpu(pd[0]).view(B, T, C) * ~own).any())
    one = torch.randn(1, B * T, C, generator=g)
    r = torch.empty(B * T, C, device=DEV)
    ops.sum_bias_act_rows(one.to(DEV), None, r, B, T, C, True)
    assert torch.equal(_cpu(r), one[0].clamp_min(0))                              # S = 1 without a bias: the plain ReLU, exact
    rep.flush()


# ------------------------------------------------------------------------------------------------ the whole model
def _store(pooling="mean+std", gating=True, idx=0, sd=None):
    cfg = W.Wav2SpkConfig(gating, K.HIDDEN, idx, pooling)
    st = W.Wav2SpkStore(cfg, DEV, num_speakers=K.SPEAKERS)
    st.load_state_dict(sd if sd is not None else K.make_state_dict(pooling=pooling))
    return st


def _device_stages(plan):
    """The stage outputs the plan holds after a step, under the names of wav2spk_cases.forward_ref."""
    out = {f"encoder.{i}": _cpu(l.y) for i, l in enumerate(plan.encoder)}
    if plan.gate:
        out["temporal_gate"] = _cpu(plan.gate.y)
    out.update({f"aggregator.{i}": _cpu(l.y) for i, l in enumerate(plan.aggregator)})
    out["pooled"] = _cpu(plan.pooled)
    out.update({f"fc.{i}": _cpu(plan.head.fc.x[i + 1]) for i in range(len(K.HIDDEN))})
    h = plan.head.head
    out["logprob"] = torch.log_softmax(_cpu(h.logits)[:, :h.C].double(), 1)
    return out


@pytest.mark.parametrize("gating,pooling", [(True, "mean+std"), (False, "mean")])
@pytest.mark.parametrize("case", K.STEP_CASES)
def test_two_train_steps_every_stage_and_gradient_vs_float64(case, gating, pooling):
    from w2v2_speaker_amd.optim.schedule import Constant
    B, N = case
    # Adam's first steps move every element by about lr whatever its gradient's size, so the elements whose gradient lies
    # below the f32 noise (a fraction of about E_ref of them) may move the other way, 2 lr apart from the float64 run: a
    # rel-L2 of about sqrt(E_ref) lr / |w|.  That stays under E_ref for lr <= |w| sqrt(E_ref), about 0.036 * 5e-3 = 1.9e-4
    # for the smallest weights (the aggregator's, He variance over 1536 inputs) at E_ref = 2.8e-5: hence 1e-4.
    lr = 1e-4
    st = _store(pooling, gating)
    plan = W.Wav2SpkPlan(st, B, N, train=True)
    tr = W.Wav2SpkTrainer(st, plan, Constant(lr, 0.9))
    wav, label = K.synth_batch(B, N)
    names = list(st.shapes)
    weights = [n for n in names if not n.endswith("bias") and n != "temporal_gate.b" and (gating or not n.startswith("temporal_gate"))]
    # the float64 run from the same start: two Adam steps of the hand-derived chain
    P64 = {n: v.double() for n, v in K.make_state_dict(pooling=pooling).items()}
    m64, v64 = {n: torch.zeros_like(v) for n, v in P64.items()}, {n: torch.zeros_like(v) for n, v in P64.items()}
    e_refs = []
    for step in (1, 2):
        P = {n: _cpu(st.p(n)).clone() for n in names}                # the parameters this step's forward and backward read
        # what torch f32 on the CPU loses against float64 on these parameters: the measure of the bounds
        rec = K.forward_ref(P, wav, label, gating, pooling)
        G = K.backward_ref(P, rec)
        rec32, G32 = K.torch_grads(P, wav, label, gating, pooling, F32)
        e_stage = max(K.rel_l2(rec32["stage"][n].detach(), t) for n, t in rec["stage"].items())
        e_ref = max(K.rel_l2(G32[n], G[n]) for n in weights)
        e_refs.append(e_ref)
        print(f"wav2spk-parity: {case} gating={gating} {pooling} step {step}: torch-f32 E_stage {e_stage:.2e} E_ref {e_ref:.2e}")
        loss, softmax = tr.train_step(wav.to(DEV), label.to(DEV))
        torch.cuda.synchronize()
        assert softmax.shape == (B, K.SPEAKERS) and tr.stepped
        rep = _Report(f"{case} gating={gating} {pooling} step {step}")
        for n, t in _device_stages(plan).items():
            rep.stage("stage output", n, t, rec["stage"][n], 2 * e_stage)
        rep.stage("loss", "", torch.tensor([float(loss)]), rec["loss"].view(1), 2 * e_stage * float(rec["logprob"].norm()) / math.sqrt(B) / float(rec["loss"]))
        for n in names:
            got = _cpu(st.g(n))
            if n.startswith("encoder.") and n.endswith("bias"):
                assert float(got.abs().max()) == 0.0, n                            # exact zeros, not rounding noise
                continue
            rep.stage("gradient", n, got, G[n], 2 * e_ref)
        rep.flush()
        # the float64 run advances on its own parameters
        rec64 = K.forward_ref(P64, wav, label, gating, pooling)
        G64 = K.backward_ref(P64, rec64)
        P64 = {n: K.adam_ref(P64[n], G64[n], m64[n], v64[n], lr, step) for n in names}
    rep = _Report(f"{case} gating={gating} {pooling} parameters after two Adam steps", 2 * max(e_refs))
    for n in names:
        rep.stage("parameter", n, _cpu(st.p(n)), P64[n])
    rep.flush()


# ------------------------------------------------------------------------------------------------ evaluation
@pytest.mark.parametrize("pooling", K.POOLINGS)
def test_padded_batch_rows_are_bit_identical_to_the_utterance_alone(pooling):
    st = _store(pooling)
    lens = list(K.EVAL_LENGTHS)
    N = max(lens)
    g = torch.Generator().manual_seed(17)
    wav = torch.randn(len(lens), N, generator=g)
    padded = wav.clone()
    for i, n in enumerate(lens):
        padded[i, n:] = 7.0                                                       # junk past the utterance: never read
    plan = W.Wav2SpkPlan(st, len(lens), N, train=False)
    alone = [W.Wav2SpkPlan(st, 1, n, train=False) for n in lens]
    for idx in K.EMBEDDING_LAYERS:
        e = plan.embed(padded.to(DEV), lengths=lens, embedding_layer_idx=idx).clone()
        assert plan.sample_lengths == lens and bool(torch.isfinite(e).all())
        assert e.shape == (len(lens), W.Wav2SpkConfig(True, K.HIDDEN, idx, pooling).embedding_size(K.SPEAKERS))
        assert torch.equal(plan.embed(padded.to(DEV), lengths=torch.tensor(lens), embedding_layer_idx=idx), e)
        for b, n in enumerate(lens):
            one = alone[b].embed(wav[b:b + 1, :n].contiguous().to(DEV), embedding_layer_idx=idx)
            assert torch.equal(e[b:b + 1], one), (idx, b, n)
    with pytest.raises(ValueError):
        plan.embed(padded.to(DEV), lengths=[805, 1600, 100, 3200, 2399])
    with pytest.raises(NotImplementedError):
        W.Wav2SpkPlan(st, len(lens), N, train=True).forward(padded.to(DEV), lengths=lens)


# ------------------------------------------------------------------------------------------------ module
def test_module_training_step_prediction_and_trials(tmp_path):
    from w2v2_speaker_amd.data.synthetic import synth_trial_set
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import EvaluationPair
    from w2v2_speaker_amd.lightning_modules.speaker import Wav2SpkModule, Wav2SpkModuleConfig
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import SpeakerClassificationDataBatch
    meta = json.load(open(os.path.join(GOLDEN, "g23_wav2spk.json")))
    gold = np.load(os.path.join(GOLDEN, "g23_wav2spk.npz"))
    c = meta["cases"][0]
    assert c["gating"] and c["pooling"] == "mean+std"
    B, N = c["batch"], c["samples"]
    mod = Wav2SpkModule.from_config(Wav2SpkModuleConfig(), K.SPEAKERS, max_lr=1e-3, max_steps=100, gradient_clip_val=1.0)
    sd = K.make_state_dict()
    mod.load_state_dict(sd)
    wav, label = K.synth_batch(B, N)
    assert mod.generate_example_input(True, 2).shape == (2, 1, 16000)
    # embedding_layer_idx 0 (the reference's configuration): the post-ReLU output of the first hidden layer
    e = mod.compute_speaker_embedding(wav[:, None, :])
    rec, rec32 = K.forward_ref(sd, wav, label), K.forward_ref(sd, wav, label, dtype=F32)
    e_stage = max(K.rel_l2(rec32["stage"][n], t) for n, t in rec["stage"].items())
    print(f"wav2spk-parity: module: torch-f32 E_stage {e_stage:.2e}")
    assert e.shape == (B, 512) and K.rel_l2(_cpu(e), K.embedding_of(rec, 0)) <= 2 * e_stage
    assert K.rel_l2(K.strided(_cpu(e), 1024), torch.from_numpy(gold[c["tag"] + ".emb.0"])) <= 2 * e_stage
    assert torch.equal(mod.compute_speaker_embedding(wav[0]), e[:1])
    logp = mod.compute_speaker_prediction(e)
    assert logp.shape == (B, K.SPEAKERS) and K.rel_l2(_cpu(logp), rec["logprob"]) <= 2 * e_stage
    assert float((_cpu(logp).double().exp().sum(1) - 1).abs().max()) <= 1e-5        # rows sum to 1 after exp
    # the loss of a training step against the golden: |mean_b d(logprob[b, label_b])| <= |d logprob|_2 / sqrt(B)
    mod.set_optimizer(torch.optim.Adam(mod.parameters(), lr=1e-3))
    mod.set_lr_schedule({"scheduler": torch.optim.lr_scheduler.MultiStepLR(mod.configure_optimizers()[0][0], [2, 3], 0.1),
                         "interval": "step"})
    batch = SpeakerClassificationDataBatch(B, [f"u{i}" for i in range(B)], wav[:, None, :], label)
    before = mod.store.flat.clone()
    out = mod.training_step(batch)
    bound = 2 * e_stage * float(rec["logprob"].norm()) / math.sqrt(B)
    print(f"wav2spk-parity: module: loss {float(out['loss']):.8f} golden {float(gold[c['tag'] + '.loss']):.8f} bound {bound:.2e}")
    assert abs(float(out["loss"]) - float(gold[c["tag"] + ".loss"])) <= bound
    assert out["prediction"].shape == (B, K.SPEAKERS) and mod.schedule_step == 1 and not torch.equal(before, mod.store.flat)
    assert all(torch.equal(mod.state_dict()[f"encoder.{i}.0.bias"], sd[f"encoder.{i}.0.bias"]) for i in range(5))
    acc = Wav2SpkModule.from_config(Wav2SpkModuleConfig(), K.SPEAKERS, accumulate_grad_batches=2)
    acc.training_step(batch)
    assert acc.schedule_step == 0 and acc.steps == 1
    acc.training_step(batch)
    assert acc.schedule_step == 1 and acc.steps == 2
    # checkpoint round trip
    path = str(tmp_path / "wav2spk.ckpt")
    mod.save_checkpoint(path)
    other = Wav2SpkModule.from_config(Wav2SpkModuleConfig(), K.SPEAKERS)
    other.load_checkpoint(path)
    assert torch.equal(other.store.flat, mod.store.flat) and other.schedule_step == 1
    # trials over six utterances of different lengths
    _, _, keys, trials = synth_trial_set(n_speakers=3, utts_per_speaker=2, n_samples=1600, seed=4)
    g = torch.Generator().manual_seed(2)
    wavs = {k: torch.randn(int(torch.randint(200, 3000, (1,), generator=g)), generator=g) for k in keys}
    pairs = [EvaluationPair(bool(s), keys[i], keys[j]) for s, i, j in trials]
    got = other.evaluate_trials(pairs, wavs, quantum=800, max_batch_samples=6400, max_batch=4)
    assert isinstance(got, dict) and "eer" in got and 0.0 <= got["eer"] <= 1.0
    embs = other.compute_speaker_embeddings([wavs[k] for k in keys], quantum=800, max_batch_samples=6400, max_batch=4)
    for k, eb in zip(keys, embs):
        assert torch.equal(eb, other.compute_speaker_embedding(wavs[k])), k
