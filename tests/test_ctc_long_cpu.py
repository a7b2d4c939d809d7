"""CPU tests of the speech recognition path: the long-target CTC kernel's arithmetic restated in f32 (pair layout,
tests/ctc_long_cases.py) against the bounds the GPU test holds the kernel to, the C ABI, the host-side limits of ``ops`` and
``CtcLoss``, the tokenizer against outputs recorded from ``transformers``' ``Wav2Vec2CTCTokenizer``
(tests/golden/g24_speech.json, written by tests/golden/make_speech_goldens.py), the word error rate on hand-counted lists,
the collate, the arena of ``ParamStore(head="letter")`` and the module's constructor errors.  Nothing here needs a GPU."""
import ctypes as C
import inspect
import json
import os

import pytest
import torch

import ctc_cases as CC
import ctc_long_cases as LC
from test_fbank_cpu import _c_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("name", LC.CASES)
def test_f32_restatement_of_the_pair_layout_meets_the_bounds(name):
    c = LC.case(name)            # (asserts that float64 is finite, and feasible exactly where the case means it to be)
    got = LC.kernel_f32_pairs(c["logits"], c["targets"], c["in_len"], c["tgt_len"], c["blank"])
    e = LC.errors(c, got["loss_rows"], got["grad"])
    print(f"ctc-long-parity (cpu restatement): {name}: loss_rows {e['loss_rows']:.3e}, grad {e['grad']:.3e}, bound "
          f"{LC.grad_bound(name):.3e}, torch_f32 {LC.ref_f32_error(name):.3e}")
    assert LC.within_bounds(name, e), e
    assert [b for b in range(len(got["infinite"])) if bool(got["infinite"][b])] == list(c["infinite"])


def test_pair_layout_restates_the_lane_layout_at_short_widths():
    """The two restatements run the same recursion state by state: on the short form's cases they agree to the rounding of
    the posterior sums (whose order differs)."""
    for name in ("repeats", "full_lattice", "mixed_bias100"):
        c = CC.case(name)
        a = CC.kernel_f32(c["logits"], c["targets"], c["in_len"], c["tgt_len"], c["blank"])
        b = LC.kernel_f32_pairs(c["logits"], c["targets"], c["in_len"], c["tgt_len"], c["blank"])
        assert torch.equal(a["loss_rows"], b["loss_rows"]) and torch.equal(a["infinite"], b["infinite"])
        assert CC.per_utterance_rel_l2(b["grad"], a["grad"].to(F64)) < 1e-6


def test_stage_cases_sit_around_the_library_s_chunk():
    n = LC.stage_frames(LC.STAGE_W)
    assert n >= 2 and [LC.case(f"stage_{s}")["logits"].shape[1] for s in ("m1", "0", "p1", "2p1")] == [n - 1, n, n + 1, 2 * n + 1]


def test_new_symbols_declared_exported_and_wrapped_with_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    from w2v2_speaker_amd import _build, _lib, ops
    kind = {C.c_void_p: "p", C.c_int64: "i64", C.c_int32: "i32", C.c_float: "f32"}
    for name in ("w2v2_ctc_long_fwd_bwd", "w2v2_ctc_greedy_decode", "w2v2_ctc_long_stage_frames"):
        assert name in _lib._SIGS and name in _lib.EXPORTS, name
        res, args = _lib._SIGS[name]
        assert res is C.c_int32 and [kind[a] for a in args] == _c_params(hdr, name), name
    res, args = _lib._SIGS["w2v2_ctc_long_workspace_floats"]
    assert res is C.c_int64 and args == [C.c_int32] * 3
    assert "int64_t w2v2_ctc_long_workspace_floats(int B, int T, int target_width);" in hdr
    # the long entry takes the argument list of the short one
    assert _lib._SIGS["w2v2_ctc_long_fwd_bwd"] == _lib._SIGS["w2v2_ctc_fwd_bwd"]
    assert _c_params(hdr, "w2v2_ctc_long_fwd_bwd") == _c_params(hdr, "w2v2_ctc_fwd_bwd")
    lib = _lib.load()
    assert "ctc_long.hip" in _build.SOURCES and "ctc_common.h" in _build.HEADERS
    assert ops.CTC_LONG_MAX_TARGET == 1023 and ops.CTC_MAX_TARGET == 31
    assert lib.w2v2_ctc_long_workspace_floats(8, 1000, 400) == ops.ctc_long_workspace_floats(8, 1000, 400) > 0
    assert ops.ctc_long_workspace_floats(2, 3, 32) > 0 and ops.ctc_long_workspace_floats(2, 3, 1023) > 0
    assert lib.w2v2_ctc_long_workspace_floats(2, 3, 1024) == -1 and lib.w2v2_ctc_long_workspace_floats(0, 3, 1) == -1
    with pytest.raises(ValueError, match="1023"):
        ops.ctc_long_workspace_floats(2, 3, 1024)
    with pytest.raises(ValueError, match="31"):
        ops.ctc_workspace_floats(2, 3, 32)                       # the short form is as it was
    # alpha and the posterior share their place: 8 bytes per state and frame, where the short layout holds 16
    assert ops.ctc_long_workspace_floats(8, 1000, 400) * 4 < 80e6
    assert ops.ctc_long_stage_frames(1023) >= 2 and ops.ctc_long_stage_frames(0) > ops.ctc_long_stage_frames(1023)
    with pytest.raises(ValueError):
        ops.ctc_long_stage_frames(1024)
    assert list(inspect.signature(ops.ctc_long_fwd_bwd).parameters) == list(inspect.signature(ops.ctc_fwd_bwd).parameters)
    assert list(inspect.signature(ops.ctc_greedy_decode).parameters) == ["logits", "input_lengths", "tokens", "counts", "B",
                                                                         "T", "C", "ldc", "blank"]


def test_loss_module_limits():
    from w2v2_speaker_amd.optim.loss import CtcLoss
    from w2v2_speaker_amd.optim.loss.ctc_loss import pad_targets
    assert CtcLoss().long_targets is False and CtcLoss(long_targets=True).long_targets is True
    assert CtcLoss(3, True).blank_idx == 3
    tl = torch.tensor([2, 0, 3], dtype=torch.int32)
    with pytest.raises(ValueError, match="at most 31"):
        CtcLoss()(torch.zeros(3, 40, 8), tl, torch.ones(3, 32, dtype=torch.int64), tl)
    with pytest.raises(ValueError, match="at most 31"):
        pad_targets(torch.ones(3, 32, dtype=torch.int64), tl, 3)
    # both layouts pass the host checks of the long form and give the kernel the same rows
    wide = torch.arange(1, 3 * 33 + 1).view(3, 33)
    lens = torch.tensor([33, 0, 5], dtype=torch.int32)
    flat = torch.cat([wide[b, :int(L)] for b, L in enumerate(lens)])
    a, b = pad_targets(wide, lens, 3, long_targets=True), pad_targets(flat, lens, 3, long_targets=True)
    assert a.shape == (3, 33) and b.shape == (3, flat.numel())          # (1-D: as wide as all labels, no synchronisation)
    for r, L in enumerate(lens.tolist()):
        assert a[r, :L].tolist() == b[r, :L].tolist()
    assert pad_targets(torch.ones(2, 1023, dtype=torch.int64), lens[:2], 2, long_targets=True).shape == (2, 1023)
    with pytest.raises(ValueError, match="at most 1023"):
        pad_targets(torch.ones(2, 1024, dtype=torch.int64), lens[:2], 2, long_targets=True)
    with pytest.raises(ValueError, match="at most 1023"):
        pad_targets(torch.ones(2 * 1023 + 1, dtype=torch.int64), lens[:2], 2, long_targets=True)
    with pytest.raises(ValueError, match="at most 1023"):
        CtcLoss(long_targets=True)(torch.zeros(2, 40, 8), lens[:2], torch.ones(2, 1024, dtype=torch.int64), lens[:2])


# ------------------------------------------------------------------------------------------------------------ tokenizer
@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(GOLDEN, "g24_speech.json")))


def test_tokenizer_against_transformers(recorded):
    from w2v2_speaker_amd.tokenizer import LETTER_VOCAB_PATH, BaseTokenizer, Wav2vec2Tokenizer
    tok = Wav2vec2Tokenizer()
    assert isinstance(tok, BaseTokenizer) and tok.vocabulary_size() == recorded["vocab_size"] == 32
    assert tok.vocabulary_dictionary() == recorded["vocab"] and tok.blank_token_id() == 0
    rec = dict(recorded["special_tokens_map"])
    rec.pop("word_delimiter_token", None)            # (newer ``transformers`` list it; the reference's pin does not)
    assert tok.special_tokens_dictionary() == rec
    assert list(tok.vocabulary_dictionary())[:5] == ["<pad>", "<s>", "</s>", "<unk>", "|"]
    assert "".join(list(tok.vocabulary_dictionary())[5:]) == "ETAONIHSRDLUMWCFGYPBVK'XJQZ"
    assert len(recorded["encode"]) >= 8 and len(recorded["decode"]) >= 8
    for string, ids in recorded["encode"]:
        got = tok.encode_string(string)
        assert got.dtype == torch.int32 and got.tolist() == ids, string
    for frames, text in recorded["decode"]:
        assert tok.decode_tensor(torch.tensor(frames, dtype=torch.int64)) == text, frames
    # the same tokenizer from a path and from a dict
    assert Wav2vec2Tokenizer(vocab=LETTER_VOCAB_PATH).vocab == Wav2vec2Tokenizer(vocab=dict(tok.vocab)).vocab == tok.vocab
    with pytest.raises(ValueError):
        Wav2vec2Tokenizer(vocab={"<pad>": 0, "A": 2, "|": 1})
    # the device decoder's output is already collapsed: nothing is grouped again
    assert tok.decode_ids([[7, 7, 4, 24, 0, 0], [4, 0, 0, 0, 0, 0], [9, 9, 9, 9, 9, 9]], [4, 1, 0]) == ["AA B", "", ""]
    assert tok.decode_ids(torch.tensor([[10, 6, 27, 12]]), torch.tensor([4])) == ["IT'S"]
    # collapse then drop, on raw frames: a a _ a -> "AA"
    assert tok.decode_tensor(torch.tensor([7, 7, 0, 7])) == "AA"


def test_wer_on_hand_counted_lists():
    from w2v2_speaker_amd.evaluation.speech.wer import calculate_wer
    assert calculate_wer(["THE CAT SAT"], ["THE CAT SAT"]) == 0.0
    assert calculate_wer([""], ["THE CAT SAT"]) == 1.0                                   # empty hypothesis: 3 deletions / 3
    assert calculate_wer(["THE BIG FAT CAT SAT DOWN"], ["THE CAT SAT"]) == 1.0            # insertions only: 3 / 3
    assert calculate_wer(["A B C D E F G"], ["A"]) == 6.0                                # a WER above one
    assert calculate_wer(["THE CAT SAT ON"], ["THE HAT SAT ON THE MAT"]) == pytest.approx(3 / 6)      # 1 sub + 2 del
    # a list: total edits over total reference words (not the mean of the sentences' rates)
    hyp = ["THE CAT", "HELLO THERE WORLD", "", "ONE TWO THREE FOUR"]
    ref = ["THE CAT SAT", "HELLO WORLD", "A B", "ONE THREE TWO FOUR"]
    assert calculate_wer(hyp, ref) == pytest.approx((1 + 1 + 2 + 2) / (3 + 2 + 2 + 4))
    assert calculate_wer("  A   B ", "A B") == 0.0
    with pytest.raises(ValueError):
        calculate_wer(["A"], ["A", "B"])
    with pytest.raises(ValueError):
        calculate_wer([""], [""])


def test_collate_pads_and_keeps_lengths_and_strings():
    from w2v2_speaker_amd.data import SpeechRecognitionDataBatch, SpeechRecognitionDataSample, speech_collate_fn
    from w2v2_speaker_amd.tokenizer import Wav2vec2Tokenizer
    tok = Wav2vec2Tokenizer()
    texts, ns = ["A CAT", "IT'S", "O"], [700, 1000, 400]
    lst = [SpeechRecognitionDataSample(f"k{i}", tok.encode_string(s), s, torch.full((1, n), float(i + 1)), n,
                                       torch.tensor(len(s))) for i, (s, n) in enumerate(zip(texts, ns))]
    b = speech_collate_fn(lst)
    assert isinstance(b, SpeechRecognitionDataBatch) and len(b) == 3 and b.keys == ["k0", "k1", "k2"]
    assert b.network_input.shape == (3, 1000) and b.input_lengths == ns
    for i, n in enumerate(ns):
        assert bool((b.network_input[i, :n] == i + 1).all()) and bool((b.network_input[i, n:] == 0).all())
    assert b.ground_truth.shape == (3, 5) and b.ground_truth_sequence_length.tolist() == [5, 4, 1]
    assert b.ground_truth[1].tolist() == tok.encode_string("IT'S").tolist() + [0] and b.ground_truth[2].tolist() == [8, 0, 0, 0, 0]
    assert b.ground_truth_strings == texts and set(b.side_info) == {"k0", "k1", "k2"}
    one = speech_collate_fn(lst[:1])                          # a batch of one keeps its batch dimension
    assert one.network_input.shape == (1, 700) and one.ground_truth.shape == (1, 5)
    assert b.to("cpu").ground_truth_strings == texts


def test_arena_of_the_letter_head():
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.params import ParamStore
    cfg = W2V2Config.tiny()
    H = cfg.hidden_size
    st = ParamStore(cfg, "cpu", torch.float32, head="letter", vocab_size=32)
    W, Bn = "speech_recognition_head.lm_head.weight", "speech_recognition_head.lm_head.bias"
    assert list(st.shapes)[:2] == [W, Bn] and st.shapes[W] == (32, H) and st.shapes[Bn] == (32,)
    assert st.embed_dim == st.head_in_dim == H
    ce = ParamStore(cfg, "cpu", torch.float32, head="ce", num_speakers=32, embed_dim=H)
    assert st.head_size() == ce.head_size() >= 32 * H + 32
    assert st.n_total == ce.n_total and st.grad_buckets() == ce.grad_buckets()       # the CE head's tensors, renamed
    st.init_weights(3)
    ce.init_weights(3)
    assert torch.equal(st.p(W), ce.p("fc_list.0.0.weight")) and float(st.p(Bn).abs().max()) == 0      # no [100, 0, ...] bias
    assert st.reference_parameter_order()[-2:] == [W, Bn]
    sd = st.state_dict()
    assert W in sd and Bn in sd and not any(k.startswith("fc_list.") for k in sd)
    other = ParamStore(cfg, "cpu", torch.float32, head="letter", vocab_size=32)
    other.load_state_dict(sd, strict=True, prefix_model=False)
    assert torch.equal(other.flat, st.flat)
    with pytest.raises(ValueError, match="vocab_size"):
        ParamStore(cfg, "cpu", torch.float32, head="letter")
    with pytest.raises(ValueError, match="vocab_size"):
        ParamStore(cfg, "cpu", torch.float32, head="ce", vocab_size=32)
    for pooling in ("mean+std", "mean", "first"):              # the check stands in front of every allocation of the plan
        with pytest.raises(ValueError, match="speech_wav2vec2_ctc"):
            Plan(st, 2, 4000, train=True, pooling=pooling)


def test_module_constructor_errors_fire_before_any_device_allocation():
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.lightning_modules.speech import Wav2vec2FcLetterRecognizer, Wav2vec2FcLetterRecognizerConfig
    from w2v2_speaker_amd.optim.loss import CrossEntropyLoss, CtcLoss
    from w2v2_speaker_amd.tokenizer import Wav2vec2Tokenizer
    tok = Wav2vec2Tokenizer()
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: W2V2Config.tiny())
    mk = lambda loss=lambda: CtcLoss(long_targets=True), **c: Wav2vec2FcLetterRecognizer(
        Wav2vec2FcLetterRecognizerConfig(reset_weights=True, **c), None, loss, tok, device="cpu")
    try:
        with pytest.raises(NotImplementedError, match="EmbeddingMasker"):
            mk(timestep_mask_prob=0.1)
        with pytest.raises(NotImplementedError, match="EmbeddingMasker"):
            mk(channel_mask_prob=0.05)
        with pytest.raises(ValueError, match="expected loss class"):
            mk(loss=CrossEntropyLoss)
        with pytest.raises(ValueError, match="blank"):
            mk(loss=lambda: CtcLoss(blank_idx=3, long_targets=True))
        with pytest.raises(ValueError, match="final_dropout"):
            Wav2vec2FcLetterRecognizer(Wav2vec2FcLetterRecognizerConfig(reset_weights=True), None, CtcLoss, tok,
                                       device="cpu", final_dropout=1.0)
        cfg = Wav2vec2FcLetterRecognizerConfig()
        assert (cfg.wav2vec_hunggingface_id, cfg.num_frozen_steps, cfg.timestep_mask_prob, cfg.channel_mask_width) == (
            "facebook/wav2vec2-base", 10000, 0.0, 64)             # config/network/wav2vec2_fc_letter.yaml
    finally:
        W2V2Config.from_huggingface_id = orig
