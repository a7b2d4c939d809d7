"""GPU tests of the triplet head: the kernel (w2v2_triplet_fwd_bwd) against the float64 reference of
tests/triplet_cases.py, heads.TripletHead, the loss modules against the gradients the reference itself produced
(tests/golden/g21_triplet.npz), and the "triplet" / "triplet_ce" modes of Plan, SpeakerTrainer and Wav2vec2FCModule.

Bounds: the ones tests/test_heads_gpu.py holds the f32 head kernels to -- loss 2e-5 relative to max(1, |ref|); d_ap, d_an
and the gradient 1e-5 rel-L2 (the largest over the rows); rows whose reference gradient is exactly zero must be exactly
zero.  tests/test_triplet_cpu.py shows that the kernel's arithmetic restated in f32 on the CPU meets them on the same
inputs (about 3e-7 / 1e-7), so a miss here is the kernel's.  Lines that start with ``triplet-parity:`` are the measured
figures recorded in profiles/triplet_parity.txt."""
import functools
import os
import random

import numpy as np
import pytest
import torch

import triplet_cases as TC
from oracle import w2v2_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
SENT = -7.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def ops():
    from w2v2_speaker_amd import ops as o
    return o


def say(what, figures):
    print("triplet-parity: " + what + ": " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}"
                                                         for k, v in figures.items()))


@functools.lru_cache(maxsize=None)
def _ref(case, margin, *args):
    """Float64 reference (coef 1, loss scale 1) of the case ``case(*args)``: computed once, shared, never modified."""
    emb, pos, neg = case(*args)
    return TC.triplet_ref(emb, pos, neg, margin)


def launch(emb, pos, neg, margin, *, coef=1.0, loss_scale=None, demb="new", accumulate=False, ld=None):
    """One launch into sentinel-filled outputs -> dict of device tensors (+ "loss" through ops.mean)."""
    o = ops()
    B, E = emb.shape
    idx = torch.tensor([pos, neg], dtype=torch.int64, device=DEV)
    out = {n: torch.full((B,), SENT, dtype=F32, device=DEV) for n in ("d_ap", "d_an", "loss_rows")}
    out["demb"] = torch.full((B, E), SENT, dtype=F32, device=DEV) if isinstance(demb, str) else demb
    ls = None if loss_scale is None else torch.tensor([loss_scale, 0.0, 0.0, 0.0], device=DEV)
    o.triplet_fwd_bwd(emb, idx[0], idx[1], out["d_ap"], out["d_an"], out["loss_rows"], out["demb"], B, E, margin, coef,
                      accumulate, ls, ld=ld)
    out["loss"] = torch.empty((), dtype=F32, device=DEV)
    o.mean(out["loss_rows"], out["loss"])
    torch.cuda.synchronize()
    return out


def check(tag, got, ref, k=1.0):
    e = TC.errors(got, ref, k)
    say(tag, {**e, "loss_bound": TC.LOSS_TOL, "grad_bound": TC.GRAD_TOL})
    assert TC.within_bounds(e), (tag, e)
    return e


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("margin", TC.MARGINS)
@pytest.mark.parametrize("B,E", TC.SHAPES)
def test_kernel_vs_float64(B, E, margin):
    emb, pos, neg = TC.shape_case(B, E)
    got = launch(emb.to(DEV), pos, neg, margin)
    check(f"kernel {B}x{E} margin {margin}", got, _ref(TC.shape_case, margin, B, E))


@pytest.mark.parametrize("margin", TC.MARGINS)
def test_fan_in_unreferenced_and_mixed_rows(margin):
    """Row 0 collects eleven foreign terms, row 11 is named by nobody; at margin 0.3 active and inactive rows mix."""
    emb, pos, neg = TC.fan_in_case()
    ref = _ref(TC.fan_in_case, margin)
    got = launch(emb.to(DEV), pos, neg, margin)
    check(f"fan-in margin {margin} ({int(ref['active'].sum())} of {TC.FAN_B} rows active)", got, ref)
    inactive = ~ref["active"]
    if margin == 0.3:
        assert 0 < int(inactive.sum()) < TC.FAN_B
        # a row that is inactive AND named by no active anchor gets an exact zero (row 11 when it is inactive)
        assert TC.errors(got, ref)["zero_rows_ok"]
    assert torch.equal(got["loss_rows"].cpu()[inactive], torch.zeros(int(inactive.sum())))


def test_all_inactive_batch_is_exactly_zero():
    emb, pos, neg = TC.all_inactive_case()
    got = launch(emb.to(DEV), pos, neg, 1.0)
    assert float(got["loss"]) == 0.0 and torch.equal(got["loss_rows"].cpu(), torch.zeros(TC.FAN_B))
    assert torch.equal(got["demb"].cpu(), torch.zeros(TC.FAN_B, TC.FAN_E))
    check("all-inactive", got, _ref(TC.all_inactive_case, 1.0))


def test_two_launches_are_bitwise_equal():
    emb, pos, neg = TC.fan_in_case()
    a, b = launch(emb.to(DEV), pos, neg, 1.0), launch(emb.to(DEV), pos, neg, 1.0)
    for n in ("demb", "d_ap", "d_an", "loss_rows", "loss"):
        assert torch.equal(a[n], b[n]), n


def test_accumulate_adds_to_what_demb_holds():
    emb, pos, neg = TC.fan_in_case()
    ref = _ref(TC.fan_in_case, 0.3)
    pre = torch.randn(TC.FAN_B, TC.FAN_E, generator=torch.Generator().manual_seed(3))
    written = launch(emb.to(DEV), pos, neg, 0.3)["demb"]
    got = launch(emb.to(DEV), pos, neg, 0.3, demb=pre.to(DEV), accumulate=True)
    assert torch.equal(got["demb"], pre.to(DEV) + written)          # one f32 add per element, bitwise
    zero = ref["demb"].abs().sum(1) == 0
    assert bool(zero.any()) and torch.equal(got["demb"].cpu()[zero], pre[zero])    # untouched rows keep the pre-fill
    with pytest.raises(RuntimeError, match="accumulate needs the gradient output"):
        launch(emb.to(DEV), pos, neg, 0.3, demb=None, accumulate=True)


def test_coef_and_loss_scale_weigh_the_gradient_only():
    emb, pos, neg = TC.fan_in_case()
    ref = _ref(TC.fan_in_case, 1.0)
    plain = launch(emb.to(DEV), pos, neg, 1.0)
    got = launch(emb.to(DEV), pos, neg, 1.0, coef=2.0, loss_scale=8.0)
    check("coef 2, loss_scale 8", got, ref, k=16.0)
    for n in ("loss_rows", "d_ap", "d_an", "loss"):
        assert torch.equal(got[n], plain[n]), n
    assert torch.equal(got["demb"], plain["demb"] * 16.0)           # a power of two: exact


def test_forward_only_leaves_no_gradient():
    emb, pos, neg = TC.fan_in_case()
    got = launch(emb.to(DEV), pos, neg, 1.0, demb=None)
    e = TC.errors(got, _ref(TC.fan_in_case, 1.0))
    assert TC.within_bounds(e) and "demb" not in e


@pytest.mark.parametrize("E,ld", [(48, 56), (255, 256), (5, 7)])
def test_row_stride_with_nan_padding(E, ld):
    """A strided view: columns [E, ld) hold NaN and must not be read (ld % 4 == 0 with E % 4 != 0 ends the 16-byte path
    in a scalar tail inside the row; ld % 4 != 0 takes the scalar path for the whole row)."""
    labels = TC.FAN_LABELS
    emb = TC.speaker_embeddings(labels, E, 900 + E)
    pos, neg = TC.draw(labels, random.Random(E))
    TC.check_gap(emb, pos, neg, (1.0,))
    buf = torch.full((len(labels), ld), float("nan"))
    buf[:, :E] = emb
    dev = buf.to(DEV)
    got = launch(dev[:, :E], pos, neg, 1.0, ld=ld)
    check(f"stride E={E} ld={ld}", got, TC.triplet_ref(emb, pos, neg, 1.0))


def test_out_of_range_index_is_not_dereferenced():
    """The bad_label convention: NaN loss for that row, no gradient from it, every other row as if it were inactive."""
    emb, pos, neg = TC.fan_in_case()
    bad_pos, bad_neg = list(pos), list(neg)
    bad_pos[5], bad_neg[9] = TC.FAN_B, -1
    got = launch(emb.to(DEV), bad_pos, bad_neg, 1.0)
    rows = got["loss_rows"].cpu()
    assert torch.isnan(rows[[5, 9]]).all() and torch.isfinite(rows[[i for i in range(TC.FAN_B) if i not in (5, 9)]]).all()
    x = emb.to(F64)
    ok = [i for i in range(TC.FAN_B) if i not in (5, 9)]
    ref = TC.triplet_ref(emb, pos, neg, 1.0)
    g = torch.zeros(TC.FAN_B, dtype=F64)
    g[ok] = 1.0 / TC.FAN_B
    unit = lambda v: v / v.norm(dim=1, keepdim=True)
    uap, uan = unit(x - x[pos] + TC.EPS) * g[:, None], unit(x - x[neg] + TC.EPS) * g[:, None]
    want = uap - uan
    want.index_add_(0, torch.tensor(pos), -uap)
    want.index_add_(0, torch.tensor(neg), uan)
    assert bool(ref["active"].all()) and torch.isfinite(got["demb"]).all()
    assert float((got["demb"].cpu().to(F64) - want).norm() / want.norm()) < TC.GRAD_TOL


def test_zero_distance_gives_a_zero_unit_vector():
    """E = 1 with p - a = f32(eps): a - p + eps == 0 in f32, d_ap == 0 on an ACTIVE row -> no NaN, the positive term
    contributes nothing.  (In float64 the same sum is 2.5e-14, not 0: the comparison is with the f32 restatement.)"""
    emb = torch.tensor([[0.0], [1e-6], [0.5], [0.75]])
    pos, neg = [1, 0, 3, 2], [2, 2, 0, 0]
    want = TC.triplet_ref(emb, pos, neg, 1.0, dtype=F32)
    assert float(want["d_ap"][0]) == 0.0 and bool(want["active"][0])
    got = launch(emb.to(DEV), pos, neg, 1.0)
    assert float(got["d_ap"][0]) == 0.0 and torch.isfinite(got["demb"]).all() and torch.isfinite(got["loss_rows"]).all()
    assert torch.allclose(got["demb"].cpu(), want["demb"], rtol=1e-6, atol=0)


def test_triplet_head_validates_and_matches_the_kernel():
    from w2v2_speaker_amd.heads import TripletHead
    emb, pos, neg = TC.fan_in_case()
    head = TripletHead(TC.FAN_B, TC.FAN_E, emb=emb.to(DEV), margin=0.3, coef=1.0, train=True, loss_scale=None)
    loss, pred = head.forward_backward(None, (pos, neg))
    torch.cuda.synchronize()
    assert pred is None
    check("TripletHead", {"loss": loss, "loss_rows": head.loss_rows, "d_ap": head.d_ap, "d_an": head.d_an,
                          "demb": head.demb}, _ref(TC.fan_in_case, 0.3))
    for bad in ((pos[:-1], neg), (pos, neg + [0]), ([TC.FAN_B] + pos[1:], neg), (pos, [-1] + neg[1:])):
        with pytest.raises(ValueError):
            head.forward_backward(None, bad)
    # without triplets: drawn from the labels with the reference's calls of `random`
    from w2v2_speaker_amd.heads import sample_triplets
    random.seed(4)
    want = sample_triplets(TC.FAN_LABELS)
    random.seed(4)
    head.forward_backward(torch.tensor(TC.FAN_LABELS, device=DEV))
    torch.cuda.synchronize()
    check("TripletHead drawn", {"loss_rows": head.loss_rows, "d_ap": head.d_ap, "d_an": head.d_an, "demb": head.demb},
          TC.triplet_ref(emb, *want, 0.3))
    ev = TripletHead(TC.FAN_B, TC.FAN_E, emb=emb.to(DEV), margin=0.3, train=False)
    assert ev.demb is None and float(ev.forward_backward(None, (pos, neg))[0]) == float(loss)


# ------------------------------------------------------------------------------------------ loss modules vs the reference
def _golden():
    return np.load(os.path.join(GOLDEN, "g21_triplet.npz"))


def _grad_err(got, ref):
    ref = torch.from_numpy(ref)
    return float((got.detach().cpu().to(F64) - ref).norm() / ref.norm())


@pytest.mark.parametrize("seed", [3, 11, 29])
def test_loss_modules_give_the_reference_gradients(seed):
    from w2v2_speaker_amd.optim.loss import TripletCrossEntropyLoss, TripletLoss
    z = _golden()
    label = torch.from_numpy(z[f"s{seed}_label"]).to(DEV)
    for m in (1.0, 0.3):
        x = torch.from_numpy(z[f"s{seed}_emb"]).float().to(DEV).requires_grad_(True)
        random.seed(seed)
        loss = TripletLoss(margin=m)(x, label)
        loss.backward()
        want = float(z[f"s{seed}_loss_m{m}"])
        fig = {"loss": abs(float(loss) - want) / max(1.0, abs(want)), "demb": _grad_err(x.grad, z[f"s{seed}_demb_m{m}"])}
        say(f"TripletLoss seed {seed} margin {m}", fig)
        assert fig["loss"] < TC.LOSS_TOL and fig["demb"] < TC.GRAD_TOL
    for c_ce, c_t in ((1, 1), (1, 2)):
        x = torch.from_numpy(z[f"s{seed}_emb"]).float().to(DEV).requires_grad_(True)
        lg = torch.from_numpy(z[f"s{seed}_logits"]).float().to(DEV).requires_grad_(True)
        random.seed(seed)
        loss, pred = TripletCrossEntropyLoss(c_ce, c_t)(x, lg, label)
        loss.backward()
        want = float(z[f"s{seed}_loss_ce{c_ce}{c_t}"])
        fig = {"loss": abs(float(loss) - want) / max(1.0, abs(want)),
               "demb": _grad_err(x.grad, z[f"s{seed}_demb_ce{c_ce}{c_t}"]),
               "dlogits": _grad_err(lg.grad, z[f"s{seed}_dlogits_ce{c_ce}{c_t}"]),
               "prediction": float((pred.cpu().to(F64) - torch.from_numpy(z[f"s{seed}_pred_ce{c_ce}{c_t}"])).abs().max())}
        say(f"TripletCrossEntropyLoss({c_ce}, {c_t}) seed {seed}", fig)
        assert fig["loss"] < TC.LOSS_TOL and fig["demb"] < TC.GRAD_TOL and fig["dlogits"] < TC.GRAD_TOL
        assert fig["prediction"] < 2e-6                       # the softmax bound of tests/test_heads_gpu.py
    with pytest.raises(AssertionError):                      # the reference's verify_labels
        TripletLoss()(torch.zeros(3, 4, device=DEV), torch.tensor([0, 0, 1], device=DEV))


# ------------------------------------------------------------------------------------------ plan, trainer, module
B, N, C = 4, 4000, 5
POS, NEG = [1, 0, 3, 2], [2, 3, 0, 1]
MARGIN, COEF = 1.0, 2.0


def _reg():
    from w2v2_speaker_amd.config import Wav2Vec2RegularisationConfig
    return Wav2Vec2RegularisationConfig(activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0,
                                        hidden_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0)


def _store(head, dtype):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.params import ParamStore
    cfg = W2V2Config.tiny()
    st = ParamStore(cfg, DEV, dtype, head=head, num_speakers=C)
    sd = O.make_state_dict(O.OracleConfig.tiny(), 20211)
    if head != "triplet":
        sd["fc_list.0.0.weight"] = O.synth_tensor("fc_list.0.0.weight", (C, 2 * cfg.hidden_size), 20211)
        sd["fc_list.0.0.bias"] = O.synth_tensor("fc_list.0.0.bias", (C,), 20211)
    st.load_state_dict(sd)
    if st.scaler is not None:
        st.scaler[0] = 256.0
    return st


def _plan(st, coef=COEF):
    from w2v2_speaker_amd.engine import Plan
    return Plan(st, B, N, train=True, reg=_reg(), triplet_margin=MARGIN, triplet_coef=coef)


@functools.lru_cache(maxsize=None)
def _batch():
    wav, _ = O.synth_batch(B, N, C, seed=5)
    return wav, torch.tensor([0, 0, 3, 3], dtype=torch.int64)


def _head_pass(head, dtype):
    wav, label = _batch()
    st = _store(head, dtype)
    plan = _plan(st)
    plan.embed(wav.to(DEV), None, (), 0)
    loss, pred = plan.head_forward_backward(label.to(DEV), (POS, NEG) if head != "ce" else None)
    torch.cuda.synchronize()
    k = 1.0 if st.scaler is None else float(st.scaler[0])
    return plan, float(loss), pred, k


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_plan_gradients(dtype):
    """"triplet": demb is the float64 triplet gradient of the plan's own pooled embedding.  "triplet_ce" minus "ce" (same
    weights, same input): c_triplet times that gradient, and the loss is CE + c_triplet * triplet.  fp16: on
    demb / loss_scale."""
    tri, tri_loss, pred, k = _head_pass("triplet", dtype)
    assert pred is None
    ref = TC.triplet_ref(tri.emb.cpu(), POS, NEG, MARGIN, coef=COEF)
    assert int(ref["active"].sum()) > 0 and float(ref["v"].abs().min()) > TC.HINGE_GAP
    check(f"plan triplet {dtype}", {"loss": torch.tensor(tri_loss), "loss_rows": tri.triplet.loss_rows,
                                    "d_ap": tri.triplet.d_ap, "d_an": tri.triplet.d_an, "demb": tri.demb}, ref, k)
    tce, tce_loss, sm, _ = _head_pass("triplet_ce", dtype)
    ce, ce_loss, sm_ce, _ = _head_pass("ce", dtype)
    assert torch.equal(tce.emb, ce.emb) and torch.equal(tce.emb, tri.emb) and torch.equal(sm, sm_ce)
    want = k * ref["demb"]
    diff = tce.demb.cpu().to(F64) - ce.demb.cpu().to(F64)
    fig = {"demb_difference": float((diff - want).norm() / want.norm()), "grad_bound": TC.GRAD_TOL,
           "loss": abs(tce_loss - (ce_loss + COEF * float(ref["loss"]))) / max(1.0, abs(tce_loss)), "loss_bound": TC.LOSS_TOL}
    say(f"plan triplet_ce - ce {dtype}", fig)
    assert fig["demb_difference"] < TC.GRAD_TOL and fig["loss"] < TC.LOSS_TOL
    # the CE head's own gradients are what the "ce" plan leaves
    gw, gw_ce = tce.store.g("fc_list.0.0.weight").cpu().to(F64), ce.store.g("fc_list.0.0.weight").cpu().to(F64)
    assert float((gw - gw_ce).norm() / gw_ce.norm()) < 1e-6


def _trainer(head, accumulate=1, dtype=torch.float32):
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    st = _store(head, dtype)
    plan = _plan(st, coef=1.0)
    return st, plan, SpeakerTrainer(st, plan, Constant(1e-3), accumulate_grad_batches=accumulate)


ENC = "encoder.layers.1.feed_forward.output_dense.weight"


@pytest.mark.parametrize("head", ["triplet", "triplet_ce"])
def test_train_steps(head):
    wav, label = _batch()
    st, plan, tr = _trainer(head)
    before = st.mp(ENC).clone()
    losses, total = [], []
    for _ in range(6):
        loss, pred = tr.train_step(wav.to(DEV), label.to(DEV), skip_layers=(), triplets=(POS, NEG))
        losses.append(float(plan.triplet.loss_rows.mean()))               # the triplet loss itself, in both modes
        total.append(float(loss))
        if len(losses) == 1:
            assert not torch.equal(st.mp(ENC), before)                    # one step moves the encoder
            assert (pred is None) if head == "triplet" else (tuple(pred.shape) == (B, C))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(st.flat).all()) and np.isfinite(losses).all()
    say(f"trainer {head} six steps", {"first": losses[0], "last": losses[-1], "step_loss_first": total[0],
                                       "step_loss_last": total[-1]})
    assert losses[-1] < losses[0] and total[-1] < total[0]
    if head == "triplet":
        assert st.head_size() == 0 and st.step_head == st.step_body == 6
    # no triplets given: drawn from the (device) label, a batch without triplets raises before anything is enqueued
    random.seed(1)
    tr.train_step(wav.to(DEV), label.to(DEV), skip_layers=())
    with pytest.raises(ValueError, match="occur once"):
        tr.train_step(wav.to(DEV), torch.tensor([0, 0, 3, 1], device=DEV), skip_layers=())


@pytest.mark.parametrize("head", ["triplet", "triplet_ce"])
def test_accumulation_window_and_frozen_encoder(head):
    wav, label = _batch()
    st, plan, tr = _trainer(head, accumulate=2)
    before = st.mp(ENC).clone()
    tr.train_step(wav.to(DEV), label.to(DEV), skip_layers=(), triplets=(POS, NEG))
    assert not tr.stepped and torch.equal(st.mp(ENC), before)
    tr.train_step(wav.to(DEV), label.to(DEV), skip_layers=(), triplets=(POS, NEG))
    assert tr.stepped and not torch.equal(st.mp(ENC), before)
    # encoder frozen: only the head slice steps -- for "triplet" that slice is empty and nothing moves
    st, plan, tr = _trainer(head)
    flat = st.flat.clone()
    loss, pred = tr.train_step_frozen_encoder(plan, wav.to(DEV), label.to(DEV), triplets=(POS, NEG))
    torch.cuda.synchronize()
    h = st.head_size()
    assert np.isfinite(float(loss)) and torch.equal(st.flat[h:], flat[h:])
    if head == "triplet":
        assert h == 0 and pred is None and (st.step_head, st.step_body) == (1, 0)
    else:
        assert h > 0 and not torch.equal(st.flat[:h], flat[:h])


def _module(loss, **kw):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import Wav2vec2FCModule, Wav2vec2FCModuleConfig
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: W2V2Config.tiny())
    try:
        cfg = Wav2vec2FCModuleConfig(reset_weights=True, attention_dropout=0.0, feat_proj_dropout=0.0, hidden_dropout=0.0,
                                     layerdrop=0.0, mask_time_prob=0.0)
        return Wav2vec2FCModule.from_config(cfg, num_speakers=C, loss=loss, device=DEV, act_dtype=torch.float32,
                                            max_lr=1e-3, max_steps=50, **kw)
    finally:
        W2V2Config.from_huggingface_id = orig


@pytest.mark.parametrize("loss", ["triplet", "triplet_ce"])
def test_module(loss, tmp_path):
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import SpeakerClassificationDataBatch
    mod = _module(loss, triplet_margin=0.5, c_triplet=2.0)
    assert (mod.loss, mod.triplet_margin, mod.c_triplet) == (loss, 0.5, 2.0 if loss == "triplet_ce" else 1.0)
    plan = mod._plan(B, N, True)
    assert (plan.triplet.margin, plan.triplet.coef) == (mod.triplet_margin, mod.c_triplet)
    wav, label = _batch()
    batch = SpeakerClassificationDataBatch(B, list("abcd"), wav, label)         # on the host: the triplets need no sync
    mod.train()
    mod.on_train_start()
    before = mod.store.mp(ENC).clone()
    out = mod.training_step(batch)
    assert set(out) == {"loss", "prediction", "train_acc"} and np.isfinite(float(out["loss"]))
    assert not torch.equal(mod.store.mp(ENC), before)
    if loss == "triplet":
        assert out["prediction"] is None and out["train_acc"] is None
    else:
        assert tuple(out["prediction"].shape) == (B, C) and 0.0 <= float(out["train_acc"]) <= 1.0
    emb, pred = mod.forward(wav)
    assert tuple(emb.shape) == (B, 2 * mod.model_cfg.hidden_size)
    assert (pred is None) if loss == "triplet" else (tuple(pred.shape) == (B, C))
    with pytest.raises(ValueError, match="occur once"):
        mod.training_step(SpeakerClassificationDataBatch(B, list("abcd"), wav, torch.tensor([0, 0, 3, 1])))
    path = str(tmp_path / "triplet.ckpt")
    mod.save_checkpoint(path)
    keys = set(torch.load(path, map_location="cpu", weights_only=True)["state_dict"])
    assert any(k.startswith("fc_list.") for k in keys) == (loss == "triplet_ce")
    from w2v2_speaker_amd.optim.loss import TripletCrossEntropyLoss, TripletLoss
    ctor = (lambda: TripletLoss(0.5)) if loss == "triplet" else (lambda: TripletCrossEntropyLoss(1, 2.0))
    orig_kw = dict(cfg=mod.cfg, num_speakers=C, device=DEV, act_dtype=torch.float32, loss_fn_constructor=ctor)
    from w2v2_speaker_amd.config import W2V2Config
    orig = W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: W2V2Config.tiny())
    try:
        back = type(mod).load_from_checkpoint(path, **orig_kw)
    finally:
        W2V2Config.from_huggingface_id = orig
    assert back.loss == loss and torch.equal(back.store.flat, mod.store.flat)
    assert back.store.step_body == mod.store.step_body == 1

