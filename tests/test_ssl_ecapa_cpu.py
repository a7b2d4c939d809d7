"""CPU tests of the wav2vec2 + ECAPA-TDNN model's host side: the float32 restatement of the layer mix against float64 on
every kernel case (the yardstick the GPU tests hold the kernels to), the formulas of the backward against autograd, the
header / ctypes table / SOURCES entries, the argument errors raised before device work, and the injection points of
Plan.backward(dmix=) for every LayerDrop pattern of a 4-layer encoder."""
import os

import pytest
import torch

import ssl_ecapa_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


@pytest.mark.parametrize("name", list(K.MIX_CASES))
def test_float32_restatement_of_the_forward_against_float64(name):
    c, fr = K.MIX_CASES[name], K.forward_reference(name)
    print(f"{K.PARITY_PREFIX} cpu forward {name}: restatement |y| err {fr['y_err']:.3e} at |y| <= {fr['y_max']:.3g}, "
          f"rstd err {fr['r_err']:.3e}")
    # the restatement is the yardstick, so it must itself be a float32-class computation: its error stays below 2^-12
    # of the output scale even where the normalisation is ill-conditioned (rstd up to 316, mean / deviation = 1000)
    assert fr["y_err"] <= 2.0 ** -12 * max(fr["y_max"], 1.0)
    y = fr["y"]
    if c["lens"] is not None:
        for b, nb in enumerate(c["lens"]):
            assert not bool(y[b, nb:].any())
    if c["norm"] and c["T"] == 1:
        assert not bool(y.any())                                  # one frame: m - mu = 0 exactly


@pytest.mark.parametrize("name", K.BWD_CASES)
def test_float32_restatement_of_the_backward_against_float64(name):
    c, br = K.MIX_CASES[name], K.backward_reference(name)
    print(f"{K.PARITY_PREFIX} cpu backward {name}: restatement dm err {br['dm_err']:.3e}, da err {br['da_err']:.3e} at "
          f"|da| <= {float(br['da'].abs().max()):.3g}")
    assert abs(float(br["da"].sum())) <= br["fold_bound"] + 1e-300
    if c["J"] == 1:
        assert float(br["da"][0]) == 0.0


@pytest.mark.parametrize("name", ["2x5x64x3", "one-logit-30", "no-instance-norm", "large-mean-channel"])
def test_backward_formulas_are_the_float64_autograd_of_the_forward(name):
    """With the exact y and rstd the header's backward is the gradient of its forward."""
    c = K.MIX_CASES[name]
    xs, a, g = K.mix_inputs(name)
    m_leaf = torch.zeros(c["B"], c["T"], c["H"], dtype=F64, requires_grad=True)
    a64 = a.to(F64).requires_grad_(True)
    y, r, w = K.mix_forward([x.to(F64) for x in xs], a64, None, c["norm"], F64)
    # d/dm through a shift of m: y(m + delta) at delta = 0
    w0 = K.softmax_weights(a, F64)
    m = sum(w0[j] * x.to(F64) for j, x in enumerate(xs)) + m_leaf
    if c["norm"]:
        d = m - m.mean(1, keepdim=True)
        y2 = d / torch.sqrt((d * d).mean(1, keepdim=True) + K.EPS)
    else:
        y2 = m
    (y2 * g.to(F64)).sum().backward()
    (y * g.to(F64)).sum().backward()
    dm, da, _ = K.mix_backward(xs, a, g, y.detach(), None if r is None else r.detach(), c["norm"], F64)
    assert float((dm - m_leaf.grad).abs().max()) <= 1e-12 * max(1.0, float(dm.abs().max()))
    assert float((da - a64.grad).abs().max()) <= 1e-11 * max(1.0, float(da.abs().max()))


def test_composed_oracle_runs_and_every_parameter_but_the_mask_embedding_gets_a_gradient():
    r64, err = K.composed_reference()
    print(f"{K.PARITY_PREFIX} cpu composed oracle f32 vs f64: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    missing = [k for k, v in r64["grads_w2v"].items() if v is None or float(v.abs().max()) == 0.0]
    assert missing == ["masked_spec_embed"], missing
    assert all(v is not None and float(v.abs().max()) > 0 for v in r64["grads_ecapa"].values())
    assert abs(float(r64["grad_a"].sum())) < 1e-12
    assert len(r64["hs"]) == 3 and r64["hs"][0].shape == (K.TINY_BATCH, 12, 64)


def test_header_ctypes_table_and_sources_have_the_layer_mix():
    from w2v2_speaker_amd import _build, _lib, ops
    header = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    for sym in ("w2v2_layer_mix_fwd", "w2v2_layer_mix_bwd", "w2v2_layer_mix_workspace_floats", "w2v2_scale_add"):
        assert sym + "(" in header and sym in _lib._SIGS, sym
    assert "layer_mix.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "layer_mix.hip"))
    assert f"#define W2V2_LAYER_MIX_MAX_STATES {ops.LAYER_MIX_MAX_STATES}" in header
    assert f"#define W2V2_LAYER_MIX_LDS_FRAMES {ops.LAYER_MIX_LDS_FRAMES}" in header
    lib = _lib.load()
    assert lib.w2v2_layer_mix_workspace_floats(66, 149, 768, 13) == 66 * 12 * 32 * 2
    for bad in ((0, 5, 64, 3), (2, 5, 60, 3), (2, 5, 64, 0), (2, 5, 64, 33)):
        assert lib.w2v2_layer_mix_workspace_floats(*bad) == -1, bad


def _states(J=3, B=2, T=5, H=64, dtype=F32):
    return [torch.zeros(B, T, H, dtype=dtype) for _ in range(J)]


class _Table:
    """What the wrappers read off a LayerMixTable, without the device copy its constructor makes."""

    def __new__(cls, J=3, rows=10, H=64):
        from w2v2_speaker_amd import ops
        t = object.__new__(ops.LayerMixTable)
        t.J, t.rows, t.H, t.dtype = J, rows, H, F32
        return t


TABLE_ERRORS = {
    "no states": lambda: [], "33 states": lambda: _states(33), "float64": lambda: _states(dtype=F64),
    "H not a multiple of 8": lambda: _states(H=60), "shapes differ": lambda: _states() + _states(1, T=6),
    "dtypes differ": lambda: _states() + _states(1, dtype=BF16), "strided": lambda: [torch.zeros(2, 5, 128)[:, :, ::2]],
    "a vector": lambda: [torch.zeros(64)],
}
WRAPPER_ERRORS = {
    "layer_mix_fwd: table": lambda o: o.layer_mix_fwd(None, torch.zeros(3), torch.zeros(10, 64), 64, 2, 5, torch.zeros(2, 64)),
    "layer_mix_fwd: B x T": lambda o: o.layer_mix_fwd(_Table(), torch.zeros(3), torch.zeros(10, 64), 64, 2, 6, torch.zeros(2, 64)),
    "layer_mix_fwd: logits": lambda o: o.layer_mix_fwd(_Table(), torch.zeros(4), torch.zeros(10, 64), 64, 2, 5, torch.zeros(2, 64)),
    "layer_mix_fwd: y is": lambda o: o.layer_mix_fwd(_Table(), torch.zeros(3), torch.zeros(10, 64, dtype=torch.float16), 64, 2, 5,
                                                     torch.zeros(2, 64)),
    "layer_mix_fwd: y needs": lambda o: o.layer_mix_fwd(_Table(), torch.zeros(3), torch.zeros(10, 64), 60, 2, 5, torch.zeros(2, 64)),
    "layer_mix_fwd: instance_norm": lambda o: o.layer_mix_fwd(_Table(), torch.zeros(3), torch.zeros(10, 64), 64, 2, 5, None),
    "layer_mix_fwd: lens": lambda o: o.layer_mix_fwd(_Table(), torch.zeros(3), torch.zeros(10, 64), 64, 2, 5, torch.zeros(2, 64),
                                                     lens=torch.zeros(2, dtype=torch.int64)),
    "layer_mix_fwd: w_out": lambda o: o.layer_mix_fwd(_Table(), torch.zeros(3), torch.zeros(10, 64), 64, 2, 5, torch.zeros(2, 64),
                                                      w_out=torch.zeros(2)),
    "layer_mix_fwd: more than": lambda o: o.layer_mix_fwd(_Table(rows=600), torch.zeros(3), torch.zeros(600, 64), 64, 1, 600,
                                                          torch.zeros(1, 64)),
    "layer_mix_bwd: dm": lambda o: o.layer_mix_bwd(_Table(), torch.zeros(3), torch.zeros(10, 64), 64, torch.zeros(10, 64), 64,
                                                   torch.zeros(2, 64), torch.zeros(10, 32), torch.zeros(3), torch.zeros(128), 2, 5),
    "layer_mix_bwd: g and y": lambda o: o.layer_mix_bwd(_Table(), torch.zeros(3), torch.zeros(10, 64), 64,
                                                        torch.zeros(10, 64, dtype=BF16), 64, torch.zeros(2, 64),
                                                        torch.zeros(10, 64), torch.zeros(3), torch.zeros(128), 2, 5),
    "layer_mix_bwd: grad_logits": lambda o: o.layer_mix_bwd(_Table(), torch.zeros(3), torch.zeros(10, 64), 64, torch.zeros(10, 64), 64,
                                                            torch.zeros(2, 64), torch.zeros(10, 64), torch.zeros(2), torch.zeros(128), 2, 5),
    "layer_mix_bwd: workspace": lambda o: o.layer_mix_bwd(_Table(), torch.zeros(3), torch.zeros(10, 64), 64, torch.zeros(10, 64), 64,
                                                          torch.zeros(2, 64), torch.zeros(10, 64), torch.zeros(3), torch.zeros(127), 2, 5),
    "scale_add: G is": lambda o: o.scale_add(torch.zeros(16, dtype=F64), torch.zeros(16), torch.zeros(3), 0, 0, True),
    "scale_add: G and dm are": lambda o: o.scale_add(torch.zeros(16), torch.zeros(24), torch.zeros(3), 0, 0, True),
    "scale_add: w is": lambda o: o.scale_add(torch.zeros(16), torch.zeros(16), torch.zeros(3, dtype=F64), 0, 0, True),
    "scale_add: 0 <= lo": lambda o: o.scale_add(torch.zeros(16), torch.zeros(16), torch.zeros(3), 1, 3, True),
}


@pytest.mark.parametrize("what", list(TABLE_ERRORS))
def test_layer_mix_table_refuses_bad_states_before_any_device_work(what):
    from w2v2_speaker_amd import ops
    with pytest.raises(ValueError) as e:
        ops.LayerMixTable(TABLE_ERRORS[what]())
    assert str(e.value).startswith("layer_mix_table:"), str(e.value)


@pytest.mark.parametrize("starts", list(WRAPPER_ERRORS))
def test_layer_mix_wrappers_raise_value_errors_that_name_them_before_any_launch(starts):
    from w2v2_speaker_amd import ops
    with pytest.raises(ValueError) as e:
        WRAPPER_ERRORS[starts](ops)
    assert str(e.value).startswith(starts), str(e.value)


def test_plan_backward_dmix_argument_rules():
    from w2v2_speaker_amd.engine import mix_backward_check
    ok = dict(train=True, stable=False, scaler=None, B=2, T=12, H=64, L=2, dmix=torch.zeros(2, 12, 64), mix_weights=torch.zeros(3))
    mix_backward_check(**ok)
    mix_backward_check(**{**ok, "dmix": None, "mix_weights": None, "stable": True})       # not this form: nothing to check
    for bad in (dict(mix_weights=None), dict(dmix=None), dict(dhidden=torch.zeros(2, 12, 64)), dict(demb=torch.zeros(2, 128)),
                dict(train=False), dict(dmix=torch.zeros(2, 11, 64)), dict(dmix=torch.zeros(2, 12, 64, dtype=torch.float16)),
                dict(mix_weights=torch.zeros(2)), dict(mix_weights=torch.zeros(3, dtype=F64)),
                dict(dmix=torch.zeros(2, 12, 128)[:, :, ::2])):
        with pytest.raises(ValueError):
            mix_backward_check(**{**ok, **bad})
    with pytest.raises(NotImplementedError, match="do_stable_layer_norm"):
        mix_backward_check(**{**ok, "stable": True})
    with pytest.raises(NotImplementedError, match="f16"):
        mix_backward_check(**{**ok, "scaler": torch.zeros(8)})


def test_model_and_trainer_limits_are_raised_before_anything_is_allocated():
    from w2v2_speaker_amd import ssl_ecapa as S
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.ecapa import EcapaConfig, EcapaPlan, EcapaStore
    from w2v2_speaker_amd.params import ParamStore
    cfg = W2V2Config.tiny()
    ecfg = EcapaConfig(input_mel_coefficients=cfg.hidden_size, lin_neurons=24, channels=(64, 64, 64, 64, 192),
                       attention_channels=16, res2net_scale=4, se_channels=16)
    enc = ParamStore(cfg, "cpu", F32, head=None, num_speakers=1)
    good = EcapaStore(ecfg, "cpu", F32, num_speakers=4, feature_weight=cfg.num_hidden_layers + 1)
    assert good.shapes["feature_weight"] == (3,) and list(good.shapes)[-1] == "feature_weight"
    assert not bool(good.p("feature_weight").any())
    good.init_weights()
    assert not bool(good.p("feature_weight").any()) and "feature_weight" in good.state_dict()
    plain = EcapaStore(ecfg, "cpu", F32, num_speakers=4)
    assert "feature_weight" not in plain.shapes and plain.n_total < good.n_total       # only when the model asks for it
    S.check_stores(enc, good, train=True)
    with pytest.raises(ValueError, match="feature_weight"):
        S.check_stores(enc, plain, train=True)
    with pytest.raises(ValueError, match="feature_weight"):
        EcapaStore(ecfg, "cpu", F32, num_speakers=4, feature_weight=33)
    with pytest.raises(ValueError, match="input_mel_coefficients"):
        S.check_stores(enc, EcapaStore(EcapaConfig.tiny(), "cpu", F32, num_speakers=4, feature_weight=3), train=True)
    with pytest.raises(NotImplementedError, match="f16"):
        S.check_stores(ParamStore(cfg, "cpu", torch.float16, head=None, num_speakers=1), good, train=True)
    S.check_stores(ParamStore(cfg, "cpu", torch.float16, head=None, num_speakers=1), good, train=False)
    import dataclasses
    stable = ParamStore(dataclasses.replace(cfg, do_stable_layer_norm=True), "cpu", F32, head=None, num_speakers=1)
    with pytest.raises(NotImplementedError, match="do_stable_layer_norm"):
        S.check_stores(stable, good, train=True)
    with pytest.raises(ValueError, match="input_grad"):
        EcapaPlan(good, 2, 12, train=False, input_grad=True)
    for kw in (dict(process_group=object()), dict(accumulate_grad_batches=2), dict(gradient_clip_val=1.0)):
        with pytest.raises(NotImplementedError, match="process_group, accumulate_grad_batches > 1 and gradient_clip_val > 0"):
            S.SslEcapaTrainer(None, None, **kw)


@pytest.mark.parametrize("group", [1, 2, 4])
@pytest.mark.parametrize("grouped", [True, False])
def test_injection_points_for_every_layerdrop_pattern_of_a_four_layer_encoder(grouped, group):
    """Every j in 0 .. L is injected exactly once; the add that carries j runs before the chain of layer j - 1 starts (and
    after the chain of every layer >= j has finished its data-gradient product), and the first add overwrites."""
    from w2v2_speaker_amd.engine import encoder_backward_schedule, mix_injection_points
    L = 4
    for skip in K.layerdrop_patterns(L):
        ev = encoder_backward_schedule(L, skip, {3, 1}, grouped, group)
        pts = mix_injection_points(ev, L)
        seen = [j for _, lo, hi, _ in pts for j in range(lo, hi + 1)]
        assert sorted(seen) == list(range(L + 1)), (skip, pts)
        assert [p[3] for p in pts] == [True] + [False] * (len(pts) - 1) and pts[0][2] == L, (skip, pts)
        assert [p[0] for p in pts] == sorted(p[0] for p in pts)
        body = {e[1]: i for i, e in enumerate(ev) if e[0] == "body"}
        dx = {e[1]: i for i, e in enumerate(ev) if e[0] == "dx"}
        assert set(body) == set(range(L)) - set(skip)
        for at, lo, hi, _ in pts:
            for j in range(lo, hi + 1):
                below = [l for l in body if l < j]          # X[j] feeds the nearest layer below that runs
                if below:
                    assert at <= body[max(below)], (skip, j, at)       # never after the chain of the layer below has started
                above = [l for l in body if l >= j]         # what flows down from above passes through these first
                for l in above:
                    assert at > dx[l], (skip, j, at, l)
