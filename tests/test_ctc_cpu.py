"""CPU tests of the CTC loss: the float64 reference of tests/ctc_cases.py against goldens the reference's own CtcLoss and
training step produced (tests/golden/g22_ctc.npz, written by tests/golden/make_ctc_goldens.py), the kernel's arithmetic
restated in f32 against the bounds the GPU test holds the kernel to, the C ABI, the constructor errors and the arena of
``ParamStore(head="ctc")``.  Nothing here needs a GPU."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import ctc_cases as CC
from test_fbank_cpu import _c_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "g22_ctc.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "g22_ctc.json")))
    return {k: torch.from_numpy(g[k]) for k in g.files}, meta


def test_float64_reference_reproduces_the_reference_class(golden):
    g, meta = golden
    z, tg, il, tl = g["generic_logits"], g["generic_targets"], g["generic_in_len"], g["generic_tgt_len"]
    ref = CC.ctc_ref(z, tg, il, tl, meta["blank"], F64)
    for layout in ("2d", "1d"):                       # the reference gives the same numbers for both layouts
        assert abs(float(ref["loss"]) - float(g[f"generic_{layout}_loss"])) < 1e-12
        assert float((ref["grad"] - g[f"generic_{layout}_grad"]).abs().max()) < 1e-13
    assert [b for b in range(len(tl)) if bool(ref["infinite"][b])] == meta["generic_infeasible"]
    assert bool((g["generic_2d_grad"][meta["generic_infeasible"][0]] == 0).all())
    # the speaker step: targets label + 1, one per utterance, every frame of every utterance
    B, T, _ = g["step_logits"].shape
    ref = CC.ctc_ref(g["step_logits"], (g["step_label"] + 1)[:, None], torch.full((B,), T, dtype=torch.int32),
                     torch.ones(B, dtype=torch.int32), 0, F64)
    assert meta["label_after_step"] == (g["step_label"] + 1).tolist()          # what the reference did to the batch
    assert abs(float(ref["loss"]) - float(g["step_loss"])) < 1e-12
    assert float((ref["grad"] - g["step_grad"]).abs().max()) < 1e-13
    logits = torch.nn.functional.linear(g["step_embedding"], g["step_weight"], g["step_bias"])
    assert float((logits - g["step_logits"]).abs().max()) < 1e-12
    assert g["step_bias"].tolist() == [100.0] + [0.0] * (meta["classes"] - 1) and meta["classes"] == meta["speakers"] + 1


@pytest.mark.parametrize("name", CC.CASES)
def test_f32_restatement_of_the_kernel_meets_the_bounds(name):
    c = CC.case(name)
    got = CC.ctc_ref(c["logits"], c["targets"], c["in_len"], c["tgt_len"], c["blank"], F32)
    e = CC.errors(c, got["loss_rows"], got["grad"])
    print(f"ctc-parity (cpu restatement): {name}: loss_rows {e['loss_rows']:.3e}, grad {e['grad']:.3e}, bound "
          f"{CC.grad_bound(name):.3e}, torch_f32 {CC.ref_f32_error(name):.3e}")
    assert CC.within_bounds(name, e), e
    assert [b for b in range(len(got["infinite"])) if bool(got["infinite"][b])] == list(c["infinite"])


def test_restatement_on_the_goldens(golden):
    g, meta = golden
    got = CC.ctc_ref(g["generic_logits"].float(), g["generic_targets"], g["generic_in_len"], g["generic_tgt_len"], 0, F32)
    ref = g["generic_2d_grad"]
    assert CC.per_utterance_rel_l2(got["grad"], ref) < CC.GRAD_TOL
    assert abs(float(got["loss"]) - float(g["generic_2d_loss"])) < CC.LOSS_TOL * max(1.0, float(g["generic_2d_loss"]))


def test_new_symbols_declared_exported_and_wrapped_with_matching_signatures():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    from w2v2_speaker_amd import _build, _lib, ops
    kind = {C.c_void_p: "p", C.c_int64: "i64", C.c_int32: "i32", C.c_float: "f32"}
    name = "w2v2_ctc_fwd_bwd"
    assert name in _lib._SIGS and name in _lib.EXPORTS
    res, args = _lib._SIGS[name]
    assert res is C.c_int32 and [kind[a] for a in args] == _c_params(hdr, name)
    res, args = _lib._SIGS["w2v2_ctc_workspace_floats"]
    assert res is C.c_int64 and args == [C.c_int32] * 3 and "int64_t w2v2_ctc_workspace_floats(int B, int T, int" in hdr
    lib = _lib.load()
    assert hasattr(lib, name) and "ctc.hip" in _build.SOURCES
    assert lib.w2v2_ctc_workspace_floats(66, 149, 1) == ops.ctc_workspace_floats(66, 149, 1) > 0
    assert lib.w2v2_ctc_workspace_floats(2, 3, 32) == -1 and lib.w2v2_ctc_workspace_floats(0, 3, 1) == -1
    with pytest.raises(ValueError, match="31"):
        ops.ctc_workspace_floats(2, 3, 32)
    assert list(inspect.signature(ops.ctc_fwd_bwd).parameters) == [
        "logits", "targets", "input_lengths", "target_lengths", "loss_rows", "dlogits", "workspace", "B", "T", "C", "ldc",
        "target_width", "target_stride", "target_offset", "blank", "loss_scale"]


def test_loss_module_keeps_the_reference_surface():
    from w2v2_speaker_amd.optim.loss import CtcLoss
    from w2v2_speaker_amd.optim.loss.ctc_loss import pad_targets
    assert CtcLoss().blank_idx == 0 and CtcLoss(blank_idx=3).blank_idx == 3
    assert list(inspect.signature(CtcLoss.forward).parameters) == ["self", "predictions", "prediction_lengths",
                                                                   "ground_truths", "ground_truth_lengths"]
    # both target layouts give the kernel the same rows (up to the columns nobody reads)
    tl = torch.tensor([2, 0, 3], dtype=torch.int32)
    two = torch.tensor([[4, 5, 9], [9, 9, 9], [1, 2, 3]])
    one = torch.tensor([4, 5, 1, 2, 3])
    a, b = pad_targets(two, tl, 3), pad_targets(one, tl, 3)
    for r, L in enumerate(tl.tolist()):
        assert a[r, :L].tolist() == b[r, :L].tolist()
    assert pad_targets(torch.zeros(0, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), 3) is None
    with pytest.raises(ValueError, match="at most 31"):
        pad_targets(torch.ones(3, 32, dtype=torch.int64), tl, 3)
    with pytest.raises(ValueError, match="at most 31"):
        pad_targets(torch.ones(3 * 31 + 1, dtype=torch.int64), tl, 3)
    with pytest.raises(ValueError):
        CtcLoss()(torch.zeros(3, 4), tl, two, tl)


def test_module_constructor_errors_fire_before_any_device_allocation():
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import Wav2vec2FCModule, Wav2vec2FCModuleConfig
    from w2v2_speaker_amd.optim.loss import CtcLoss
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: W2V2Config.tiny())
    mk = lambda **kw: Wav2vec2FCModule.from_config(Wav2vec2FCModuleConfig(reset_weights=True, **kw), 4, loss="ctc",
                                                   device="cpu")
    try:
        for pooling in ("mean+std", "mean", "first+cls"):
            with pytest.raises(ValueError, match="speaker_wav2vec2_ctc"):
                mk(stat_pooling_type=pooling)
        with pytest.raises(NotImplementedError, match="embedding_layer_idx"):
            mk(stat_pooling_type="none", hidden_fc_layers_out=[16], embedding_layer_idx=0)
        with pytest.raises(NotImplementedError, match="blank_idx"):
            Wav2vec2FCModule(None, Wav2vec2FCModuleConfig(reset_weights=True, stat_pooling_type="none"), 4,
                             lambda: CtcLoss(blank_idx=2), device="cpu")
    finally:
        W2V2Config.from_huggingface_id = orig


def test_arena_of_the_ctc_head():
    """What "ce" owns with one more row (class 0 = blank), the reference's bias initialisation, the CE head's checkpoint
    keys through the store's own save / load."""
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.params import ParamStore
    cfg = W2V2Config.tiny()
    mk = lambda head, n=7, **kw: ParamStore(cfg, "cpu", torch.float32, head=head, num_speakers=n, embed_dim=cfg.hidden_size,
                                            **kw)
    ctc, ce = mk("ctc", hidden_fc=(16,)), mk("ce", 8, hidden_fc=(16,))
    assert ctc.shapes["fc_list.1.0.weight"] == (8, 16) and ctc.shapes["fc_list.1.0.bias"] == (8,)
    assert list(ctc.shapes.items()) == list(ce.shapes.items()) and ctc.offsets == ce.offsets
    assert ctc.head_size() == ce.head_size() > 0 and ctc.grad_buckets() == ce.grad_buckets()
    assert ctc.reference_parameter_order() == ce.reference_parameter_order()
    ctc.init_weights(3)
    ce.init_weights(3)
    assert ctc.p("fc_list.1.0.bias").tolist() == [100.0] + [0.0] * 7          # ref: wav2vec2_fc.py:226-233
    assert ctc.p("fc_list.0.0.bias").abs().max() == 0 and ce.p("fc_list.1.0.bias").abs().max() == 0
    assert torch.equal(ctc.p("fc_list.1.0.weight"), ce.p("fc_list.1.0.weight"))      # the Linear's default init
    sd = ctc.state_dict()
    assert set(sd) == set(ce.state_dict())
    other = mk("ctc", hidden_fc=(16,))
    other.load_state_dict(sd, strict=True, prefix_model=False)
    assert torch.equal(other.flat, ctc.flat)


def test_plan_of_a_ctc_store_needs_no_pooling_to_train():
    """The check stands in front of every allocation of the plan."""
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.params import ParamStore
    cfg = W2V2Config.tiny()
    st = ParamStore(cfg, "cpu", torch.float32, head="ctc", num_speakers=7, embed_dim=cfg.hidden_size)
    for pooling in ("mean+std", "mean", "first"):
        with pytest.raises(ValueError, match="speaker_wav2vec2_ctc"):
            Plan(st, 2, 4000, train=True, pooling=pooling)
