"""Golden vectors of the speech recognition path (authoring machine only; needs ``transformers`` and /root/reference).

g24_speech.json: the letter tokenizer.  ``transformers``' ``Wav2Vec2CTCTokenizer`` is built from the package's own
vocabulary file (w2v2_speaker_amd/tokenizer/letter_vocab.json) and its ids for a handful of strings, and its ``decode`` of a
handful of per-frame argmax sequences, are recorded.

g24_speech.npz: two training steps of the tiny letter recogniser in float64.  HF's ``Wav2Vec2Model`` from a tiny local
config (the geometry of g1_tiny; dropouts, LayerDrop and SpecAugment off; feature extractor frozen) with the weights of
``oracle.w2v2_oracle.make_state_dict``, an ``lm_head`` Linear onto the 32 letters, the REFERENCE's own ``CtcLoss`` class and
the letter step restated from ref: src/lightning_modules/speech/speech_recognition_module.py:100-116 with the frame
lengths of ref: src/lightning_modules/speech/wav2vec2_fc_letter.py:146.  Three utterances of different lengths, zero-padded
to one as the collate does; no attention mask, as in the reference.  Recorded: the first step's loss, logits and the
gradient of every trainable parameter (f32 is enough for the test's tolerances and keeps the file small), then -- after one
SGD step, lr 0.01, no momentum -- the second step's loss and logits.  The waveforms are not stored: the test draws them
from ``oracle.w2v2_oracle.synth_batch`` with the recorded seed and zeroes the padding.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_speech_goldens.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "src", "optim", "loss"))
from ctc_loss import CtcLoss  # noqa: E402  (the module alone: the package's __init__ pulls in the whole training stack)
from transformers import Wav2Vec2Config, Wav2Vec2Model  # noqa: E402
from transformers.models.wav2vec2 import Wav2Vec2CTCTokenizer  # noqa: E402

from oracle import w2v2_oracle as O  # noqa: E402

F64 = torch.float64
VOCAB = os.path.join(ROOT, "w2v2_speaker_amd", "tokenizer", "letter_vocab.json")

# ----------------------------------------------------------------------------------------------------------- tokenizer
tok = Wav2Vec2CTCTokenizer(VOCAB)
STRINGS = ["IT'S A CAT", " HELLO WORLD ", "A  B", "hello", "", "|A|", "DON'T STOP", "THE QUICK BROWN FOX JUMPS OVER THE LAZY D",
           "MISTER QUILTER", "AT"]
PAD, BAR, A, T_, S, APO, I_ = 0, 4, 7, 6, 12, 27, 10
FRAMES = [
    [PAD, BAR, BAR, I_, I_, PAD, I_, T_, PAD, APO, S, BAR, PAD, PAD],      # repeats across a pad, leading / trailing |
    [A, A, PAD, A],                                                       # a a _ a -> "AA"
    [BAR, A, BAR], [BAR, BAR, BAR], [PAD] * 5, [],
    [1, A, 2, 3, A],                                                      # <s> </s> <unk> are kept as text
    [APO, BAR, APO, S], [A, BAR, APO, BAR, A],                            # apostrophes next to word breaks
    [T_, T_, T_, 11, 11, PAD, 5, 5, BAR, BAR, PAD, BAR, 19, A, A, A, T_],
]
meta = {"vocab_size": tok.vocab_size, "special_tokens_map": dict(tok.special_tokens_map), "vocab": tok.get_vocab(),
        "encode": [[s, tok(s).input_ids] for s in STRINGS],
        "decode": [[f, tok.decode(torch.tensor(f, dtype=torch.int64))] for f in FRAMES],
        "transformers": __import__("transformers").__version__, "torch": torch.__version__}

# ---------------------------------------------------------------------------------------------------- two letter steps
cfg = O.OracleConfig.tiny()
hf = Wav2Vec2Config(attn_implementation="eager", conv_dim=list(cfg.conv_dim), hidden_size=cfg.hidden_size,
                    num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                    intermediate_size=cfg.intermediate_size, num_conv_pos_embeddings=cfg.num_conv_pos_embeddings,
                    num_conv_pos_embedding_groups=cfg.num_conv_pos_embedding_groups,
                    do_stable_layer_norm=cfg.do_stable_layer_norm, feat_extract_norm=cfg.feat_extract_norm,
                    conv_bias=cfg.conv_bias, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                    hidden_dropout=0.0, layerdrop=0.0, mask_time_prob=0.05, mask_feature_prob=0.0,
                    apply_spec_augment=False)      # (a non-zero mask_time_prob keeps masked_spec_embed in the model; nothing is masked)
SEED, WAV_SEED, V = 20211, 2424, 32
model = Wav2Vec2Model(hf)
model.load_state_dict(O.make_state_dict(cfg, SEED), strict=True)
model = model.double().train()
model.feature_extractor.requires_grad_(False)          # completely_freeze_feature_extractor: true
H = cfg.hidden_size
lm_head = torch.nn.Linear(H, V).double()
W_NAME, B_NAME = "speech_recognition_head.lm_head.weight", "speech_recognition_head.lm_head.bias"
with torch.no_grad():
    lm_head.weight.copy_(O.synth_tensor(W_NAME, (V, H), SEED))
    lm_head.bias.copy_(O.synth_tensor(B_NAME, (V,), SEED))

B, N = 3, 16000
samples = [16000, 13000, 9700]
texts = ["THE QUICK BROWN FOX JUMPS OVER THE LAZY D", "MISTER QUILTER IS", "AT"]
wav, _ = O.synth_batch(B, N, 2, seed=WAV_SEED)
wav = wav[:, 0, :].clone()
for b, n in enumerate(samples):
    wav[b, n:] = 0.0                                    # right-padded by the collate
ids = [tok(s).input_ids for s in texts]
gt_len = torch.tensor([len(i) for i in ids], dtype=torch.int64)
gt = torch.zeros(B, int(gt_len.max()), dtype=torch.int64)
for b, i in enumerate(ids):
    gt[b, :len(i)] = torch.tensor(i)
import math  # noqa: E402
frames = [math.floor((n - 80) / 320) for n in samples]           # ref: wav2vec2_fc_letter.py:146


def letter_step():
    emb = model(wav.double()).last_hidden_state                   # [B, T, H]; no attention mask (ref: models/wav2vec2.py)
    pred = lm_head(emb)                                           # final_dropout 0
    loss = CtcLoss()(predictions=pred, ground_truths=gt, prediction_lengths=torch.IntTensor(frames),
                     ground_truth_lengths=gt_len)
    return emb, pred, loss


params = [p for p in list(model.parameters()) + list(lm_head.parameters()) if p.requires_grad]
opt = torch.optim.SGD(params, lr=0.01)
out = {}
emb, pred, loss = letter_step()
loss.backward()
out["step1_loss"], out["step1_logits"], out["step1_embedding"] = loss.detach().numpy(), pred.detach().numpy(), emb.detach().numpy()
for n, p in model.named_parameters():
    if p.requires_grad:
        out["grad.wav2vec.model." + n] = (p.grad if p.grad is not None else torch.zeros_like(p)).float().numpy()
out["grad." + W_NAME], out["grad." + B_NAME] = lm_head.weight.grad.float().numpy(), lm_head.bias.grad.float().numpy()
opt.step()
opt.zero_grad()
emb, pred, loss2 = letter_step()
out["step2_loss"], out["step2_logits"] = loss2.detach().numpy(), pred.detach().numpy()
out["targets"], out["target_lengths"] = gt.numpy(), gt_len.numpy()
meta.update({"steps": {"seed": SEED, "wav_seed": WAV_SEED, "batch": B, "padded_samples": N, "samples": samples,
                       "frames": frames, "texts": texts, "lr": 0.01, "vocab_size": V}})

np.savez_compressed(os.path.join(HERE, "g24_speech.npz"), **out)
with open(os.path.join(HERE, "g24_speech.json"), "w") as f:
    json.dump(meta, f, indent=1)
print("loss", float(loss), "->", float(loss2), "frames", frames, "targets", gt_len.tolist(), "keys", len(out),
      os.path.getsize(os.path.join(HERE, "g24_speech.npz")), "bytes")
