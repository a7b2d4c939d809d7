"""GPU tests of the speech recognition path (config/experiment/speech_wav2vec2_ctc.yaml of the reference): two training
steps of the tiny letter recogniser against tests/golden/g24_speech.npz -- HF's ``Wav2Vec2Model``, the reference's own
``CtcLoss`` and the letter step in float64, written by tests/golden/make_speech_goldens.py -- and the
``Wav2vec2FcLetterRecognizer`` module over the same weights.

Tolerances: the ones tests/test_parity_gpu.py::test_tiny_all_stages_loss_and_every_gradient_vs_reference_golden holds the
tiny speaker step to, per precision mode (its lines 82-102), named here."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import w2v2_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# test_parity_gpu.py: `tol` (stage activations, rel-L2), the loss factor, `gtol` and `floor` (every gradient)
STAGE_TOL = {F32: 1e-4, F16: 3e-3, BF16: 3e-2}
LOSS_TOL = {F32: 1e-4, F16: 2e-3, BF16: 5e-2}
GRAD_TOL = {F32: 2e-3, F16: 6e-3, BF16: 0.12}
GRAD_FLOOR = {F32: 1e-6, F16: 2e-4, BF16: 2e-3}
W_HEAD, B_HEAD = "speech_recognition_head.lm_head.weight", "speech_recognition_head.lm_head.bias"


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "g24_speech.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "g24_speech.json")))["steps"]
    wav, _ = O.synth_batch(meta["batch"], meta["padded_samples"], 2, seed=meta["wav_seed"])
    wav = wav[:, 0, :].clone()
    for b, n in enumerate(meta["samples"]):
        wav[b, n:] = 0.0
    return g, meta, wav


def _state_dict(meta):
    cfg = O.OracleConfig.tiny()
    sd = O.make_state_dict(cfg, meta["seed"])
    V = meta["vocab_size"]
    sd[W_HEAD] = O.synth_tensor(W_HEAD, (V, cfg.hidden_size), meta["seed"])
    sd[B_HEAD] = O.synth_tensor(B_HEAD, (V,), meta["seed"])
    return sd


def _no_reg():
    from w2v2_speaker_amd.config import Wav2Vec2RegularisationConfig
    return Wav2Vec2RegularisationConfig(activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                                        hidden_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0)


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_two_letter_steps_against_the_float64_golden(golden, dtype):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim import OptimConfig
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.params import ParamStore
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    g, meta, wav = golden
    V, B, N = meta["vocab_size"], meta["batch"], meta["padded_samples"]
    st = ParamStore(W2V2Config.tiny(), DEV, dtype, head="letter", vocab_size=V)
    st.load_state_dict(_state_dict(meta))
    if st.scaler is not None:
        st.scaler[0] = 256.0
    plan = Plan(st, B, N, train=True, reg=_no_reg(), pooling="none", max_target=64)
    assert plan.T == max(meta["frames"]) and plan.frames_of(meta["samples"]) == meta["frames"]
    tr = SpeakerTrainer(st, plan, Constant(meta["lr"], 0.0), optimizer=OptimConfig(algo="sgd", momentum=0.0))
    transcript = (torch.from_numpy(g["targets"]), torch.from_numpy(g["target_lengths"]), meta["samples"])
    x = wav.to(DEV)
    loss1, pred = tr.train_step(x, None, skip_layers=(), transcript=transcript)
    torch.cuda.synchronize()
    assert pred is None and plan.head.width == g["targets"].shape[1] > 31          # the long kernels ran
    T = plan.T
    fig = {"loss": abs(float(loss1) - float(g["step1_loss"])) / abs(float(g["step1_loss"])),
           "embedding": rel_l2(plan.emb.float().cpu().view(B, T, -1), g["step1_embedding"]),
           "logits": rel_l2(plan.head.logits[:, :V].cpu().view(B, T, V), g["step1_logits"])}
    gs = float(st.scaler[0]) if st.scaler is not None else 1.0
    worst = 0.0
    for name in st.shapes:
        if not st.is_trainable(name):
            continue
        ref = g["grad." + name].astype(np.float64)
        got = st.g(name).cpu().numpy().astype(np.float64) / gs
        err = np.linalg.norm(got - ref)
        assert err <= GRAD_TOL[dtype] * np.linalg.norm(ref) + GRAD_FLOOR[dtype], (name, err, np.linalg.norm(ref))
        # (the figure leaves out the gradients that are zero but for rounding: masked_spec_embed -- nothing is masked --
        #  and the key biases, to which a softmax row is invariant; the assertion above holds them to the floor)
        if np.linalg.norm(ref) > 1e-6:
            worst = max(worst, err / np.linalg.norm(ref))
    fig["worst_grad"] = worst
    loss2, _ = tr.train_step(x, None, skip_layers=(), transcript=transcript)
    torch.cuda.synchronize()
    fig["loss2"] = abs(float(loss2) - float(g["step2_loss"])) / abs(float(g["step2_loss"]))
    fig["logits2"] = rel_l2(plan.head.logits[:, :V].cpu().view(B, T, V), g["step2_logits"])
    print(f"speech-parity: two letter steps {dtype}: " + ", ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    assert fig["loss"] < LOSS_TOL[dtype] and fig["loss2"] < LOSS_TOL[dtype]
    assert max(fig["embedding"], fig["logits"], fig["logits2"]) < STAGE_TOL[dtype]


def _python_transcriptions(pred, frames, tokenizer):
    """ref: speech_recognition_module.py:233-248: an argmax per utterance, then the tokenizer's decode."""
    return [tokenizer.decode_tensor(torch.argmax(pred[b, :frames[b]], dim=1).cpu()) for b in range(pred.shape[0])]


def test_module(golden, tmp_path):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.data import SpeechRecognitionDataSample, speech_collate_fn
    from w2v2_speaker_amd.lightning_modules.speech import wav2vec2_fc_letter as M
    from w2v2_speaker_amd.optim.loss import CtcLoss
    from w2v2_speaker_amd.tokenizer import Wav2vec2Tokenizer
    g, meta, wav = golden
    tok = Wav2vec2Tokenizer()
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: W2V2Config.tiny())
    try:
        cfg = M.Wav2vec2FcLetterRecognizerConfig(reset_weights=True)
        kw = dict(device=DEV, act_dtype=F32, max_lr=1e-3, max_steps=50, reg=_no_reg(), max_target=64, train_wer_every=1)
        mod = M.Wav2vec2FcLetterRecognizer.from_config(cfg, tok, pretrained_state_dict=_state_dict(meta), **kw)
        samples = [SpeechRecognitionDataSample(f"utt{b}", tok.encode_string(s), s, wav[b, :n], n, torch.tensor(len(s)))
                   for b, (s, n) in enumerate(zip(meta["texts"], meta["samples"]))]
        batch = speech_collate_fn(samples)
        assert torch.equal(batch.ground_truth.to(torch.int64), torch.from_numpy(g["targets"]))
        assert torch.equal(batch.network_input, wav)
        # validation before any step: the loss of the golden's first step, the transcriptions of the Python loop
        mod.eval()
        (emb, frames), (pred, _) = mod.forward(batch.network_input, batch.input_lengths)
        assert frames == meta["frames"] and rel_l2(pred.cpu(), g["step1_logits"]) < STAGE_TOL[F32]
        out = mod.validation_step(batch)
        assert abs(float(out["val_loss"]) - float(g["step1_loss"])) < LOSS_TOL[F32] * float(g["step1_loss"])
        expect = _python_transcriptions(pred, frames, tok)
        assert out["transcription"] == expect and out["ground_truth"] == meta["texts"]
        assert mod.test_step(batch)["transcription"] == expect
        assert mod._decode_letter_prediction(pred, frames) == expect
        ends = mod.validation_epoch_end([[out], [out]])
        assert ends["val_wer_clean"] == ends["val_wer_other"] > 0 and abs(ends["val_loss_clean"] - float(out["val_loss"])) < 1e-6
        pred2, _ = mod.compute_vocabulary_prediction(emb, frames)
        assert rel_l2(pred2.cpu(), pred.cpu()) < STAGE_TOL[F32]
        # training: the same loss, then it falls
        mod.train()
        mod.on_train_start()
        loss = mod.training_step(batch, 0)
        assert abs(float(loss) - float(g["step1_loss"])) < LOSS_TOL[F32] * float(g["step1_loss"])
        assert mod.train_wer is not None and mod.plans_built == 2          # one evaluation, one training plan
        for i in range(4):
            last = mod.training_step(batch, i + 1)
        assert float(last) < float(loss) and mod.schedule_step == 5
        # a second batch of another padded length builds a second plan and evicts nothing below the cap
        short = speech_collate_fn(samples[1:])
        assert short.network_input.shape == (2, meta["samples"][1])
        l2 = mod.training_step(short, 5)
        assert np.isfinite(float(l2)) and mod.plans_built == 3 and len(mod._plans) == 3 <= M.MAX_PLANS
        assert len(mod._trainers) == 2
        # checkpoint round trip
        path = str(tmp_path / "speech.ckpt")
        mod.save_checkpoint(path)
        sd = torch.load(path, map_location="cpu", weights_only=True)["state_dict"]
        assert tuple(sd[W_HEAD].shape) == (32, 64) and tuple(sd[B_HEAD].shape) == (32,)
        back = M.Wav2vec2FcLetterRecognizer.load_from_checkpoint(
            path, cfg=cfg, loss_fn_constructor=lambda: CtcLoss(long_targets=True), tokenizer=tok, **kw)
        assert torch.equal(back.store.flat, mod.store.flat) and back.schedule_step == mod.schedule_step == 6
        assert back.store.step_body == mod.store.step_body == 6
    finally:
        W2V2Config.from_huggingface_id = orig
