"""The learned layer mix (csrc/layer_mix.hip), its injection into the encoder's backward and the wav2vec2 + ECAPA-TDNN model
on the GPU, against the float64 references of ssl_ecapa_cases.py.  Kernel bounds: 4 x the error of the float32
restatement of the header's definitions on the same case + one unit in the last place of the stored type; encoder and
ECAPA stages: the bounds test_parity_gpu.py / test_ecapa_gpu.py / test_ecapa_stages_gpu.py hold at their tiny geometries.
Figures are printed under ``ssl-ecapa-parity:`` (profiles/ssl_ecapa_parity.txt)."""
import pytest
import torch

import ecapa_stage_cases as EK
import ssl_ecapa_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENTINEL = 1024.0


def _note(msg):
    print(f"{K.PARITY_PREFIX} {msg}")


def _launch_forward(xs, a, lens, norm, ydt, pad=8):
    """One forward launch into sentinel-filled outputs -> (y_full [B*T + 1, H + pad], rstd_full [B*H + 8], w [J])."""
    from w2v2_speaker_amd import ops
    B, T, H = xs[0].shape
    gx = [x.to(DEV).contiguous() for x in xs]
    table = ops.LayerMixTable(gx)
    y_full = torch.full((B * T + 1, H + pad), SENTINEL, dtype=ydt, device=DEV)
    r_full = torch.full((B * H + 8,), SENTINEL, dtype=F32, device=DEV)
    w = torch.full((len(xs),), SENTINEL, dtype=F32, device=DEV)
    stage = torch.empty(B * T, H, dtype=F32, device=DEV) if (norm and T > ops.LAYER_MIX_LDS_FRAMES) else None
    lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    ops.layer_mix_fwd(table, a.to(DEV), y_full, H + pad, B, T, rstd=r_full[:B * H].view(B, H) if norm else None, lens=lens_dev,
                      w_out=w, stage=stage, instance_norm=norm)
    torch.cuda.synchronize()
    return y_full.cpu(), r_full.cpu(), w.cpu()


@pytest.mark.parametrize("name", list(K.MIX_CASES))
def test_forward_against_float64_writes_every_valid_element_and_nothing_else(name):
    c, fr = K.MIX_CASES[name], K.forward_reference(name)
    xs, a, _ = K.mix_inputs(name)
    B, T, H = c["B"], c["T"], c["H"]
    y_full, r_full, w = _launch_forward(xs, a, c["lens"], c["norm"], c["y"])
    y = y_full[:B * T, :H].view(B, T, H)
    assert bool((y_full[:B * T, H:] == SENTINEL).all()) and bool((y_full[B * T:] == SENTINEL).all()), "wrote beyond y"
    assert not bool((y.float() == SENTINEL).any()), "an element of y was not written"
    ok, ratio, err = K.within(y, fr["y"], fr["y_err"], c["y"])
    _note(f"gpu forward {name}: |y| err {err:.3e} (restatement {fr['y_err']:.3e}), {ratio:.2f} of the bound")
    assert ok, (name, err, fr["y_err"], ratio)
    assert float((w.double() - fr["w"]).abs().max()) <= 8 * 2.0 ** -24        # w <= 1: a few f32 roundings of exp and sum
    if c["norm"]:
        assert bool((r_full[B * H:] == SENTINEL).all())
        ok, ratio, err = K.within(r_full[:B * H].view(B, H), fr["r"], fr["r_err"], F32)
        _note(f"gpu forward {name}: rstd err {err:.3e} (restatement {fr['r_err']:.3e}), {ratio:.2f} of the bound")
        assert ok, (name, "rstd", err, fr["r_err"])
    else:
        assert bool((r_full == SENTINEL).all()), "instance_norm = false touched rstd"
    if c["special"] == "constant":
        assert float(y[:, :, 3].abs().max()) <= 4 * fr["y_err"] + 2.0 ** -126
    if c["norm"] and T == 1:
        assert not bool(y.any())
    if c["lens"] is not None:
        for b, n in enumerate(c["lens"]):
            assert not bool(y[b, n:].any()), "rows past the length are zero"
            y1, r1, _ = _launch_forward([x[b:b + 1, :n] for x in xs], a, None, c["norm"], c["y"])
            assert torch.equal(y[b, :n], y1[:n, :H]), (name, b, "not bit-equal to the utterance alone")
            if c["norm"]:
                assert torch.equal(r_full[b * H:(b + 1) * H], r1[:H])


@pytest.mark.parametrize("name", K.BWD_CASES)
def test_backward_against_float64_is_reproducible_and_adds_into_the_gradient(name):
    from w2v2_speaker_amd import ops
    c, br = K.MIX_CASES[name], K.backward_reference(name)
    xs, a, g = K.mix_inputs(name)
    B, T, H, J, norm = c["B"], c["T"], c["H"], c["J"], c["norm"]
    gx = [x.to(DEV).contiguous() for x in xs]
    table = ops.LayerMixTable(gx)
    gd, yd = g.to(DEV).view(B * T, H).contiguous(), br["y_st"].to(DEV).view(B * T, H).contiguous()
    rd = br["r_st"].to(DEV).contiguous() if norm else None
    ws = ops.layer_mix_workspace(B, T, H, J, DEV)
    ad = a.to(DEV)
    outs = []
    for start in (0.0, 0.0, 0.5):
        dm = torch.full((B * T, H), SENTINEL, dtype=F32, device=DEV)
        grad = torch.full((J,), start, dtype=F32, device=DEV)
        ops.layer_mix_bwd(table, ad, gd, H, yd if norm else None, H, rd, dm, grad, ws, B, T, instance_norm=norm)
        torch.cuda.synchronize()
        outs.append((dm.cpu(), grad.cpu()))
    (dm, da), (dm2, da2), (_, da_on_half) = outs
    assert torch.equal(dm, dm2) and torch.equal(da, da2), "two launches on the same inputs differ"
    ok, ratio, err = K.within(dm.view(B, T, H), br["dm"], br["dm_err"], F32)
    _note(f"gpu backward {name}: dm err {err:.3e} (restatement {br['dm_err']:.3e}), {ratio:.2f} of the bound")
    assert ok, (name, "dm", err, br["dm_err"])
    ok, ratio, err = K.within(da, br["da"], br["da_err"], F32)
    _note(f"gpu backward {name}: da err {err:.3e} (restatement {br['da_err']:.3e}) at |da| <= {float(br['da'].abs().max()):.3g}, "
          f"{ratio:.2f} of the bound; |sum da| {abs(float(da.double().sum())):.3e} (bound {br['fold_bound']:.3e})")
    assert ok, (name, "da", err, br["da_err"])
    assert abs(float(da.double().sum())) <= br["fold_bound"]
    if J == 1:
        assert float(da[0]) == 0.0
    ok, _, err = K.within(da_on_half, br["da"] + 0.5, br["da_err"], F32)       # ADDED to what the arena held
    assert ok, (name, "da added to 0.5", err)


@pytest.mark.parametrize("gdt,ddt", [(F32, F32), (BF16, F32), (torch.float16, F32), (BF16, BF16), (F32, BF16)])
def test_scale_add_against_float64(gdt, ddt):
    from w2v2_speaker_amd import ops
    gen = torch.Generator().manual_seed(11)
    n = 8 * 1031                                             # not a multiple of the 256-thread block
    G0, dm, w = torch.randn(n, generator=gen).to(gdt), torch.randn(n, generator=gen).to(ddt), torch.rand(5, generator=gen)
    for lo, hi, ow in ((1, 3, False), (0, 4, True), (2, 2, False)):
        G = G0.to(DEV).clone()
        ops.scale_add(G, dm.to(DEV), w.to(DEV), lo, hi, ow)
        torch.cuda.synchronize()
        s = w[lo:hi + 1].double().sum()
        ref = (0.0 if ow else G0.double()) + s * dm.double()
        # the weights' f32 sum (hi - lo roundings) times dm, one fused multiply-add, one rounding to G's dtype
        bound = (hi - lo + 1) * 2.0 ** -24 * float(s) * dm.double().abs() + K.ulp(ref, gdt)
        assert bool(((G.cpu().double() - ref).abs() <= bound).all()), (gdt, ddt, lo, hi, ow)


# ---------------------------------------------------------------------------------------- the tiny model
def _no_reg(**kw):
    from w2v2_speaker_amd.config import Wav2Vec2RegularisationConfig
    base = dict(activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, hidden_dropout=0.0, layerdrop=0.0,
                mask_time_prob=0.0)
    return Wav2Vec2RegularisationConfig(**{**base, **kw})


def _ecapa_config():
    from w2v2_speaker_amd.ecapa import EcapaConfig
    return EcapaConfig(input_mel_coefficients=64, lin_neurons=24, channels=(64, 64, 64, 64, 192), attention_channels=16,
                       res2net_scale=4, se_channels=16)


def _enc_store(dtype):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.params import ParamStore
    st = ParamStore(W2V2Config.tiny(), DEV, dtype, head=None, num_speakers=1)
    st.load_state_dict(K.tiny_state()[0])
    return st


def _ecapa_store(dtype):
    from w2v2_speaker_amd.ecapa import EcapaStore
    _, sde, fcw, a = K.tiny_state()
    st = EcapaStore(_ecapa_config(), DEV, dtype, num_speakers=K.TINY_CLASSES, feature_weight=3)
    st.load_state_dict({**sde, "loss_fn.fc_weights": fcw, "feature_weight": a})
    return st


def _enc_grads(st):
    """Trainable encoder gradients by the oracle's bare names."""
    P = "wav2vec.model."
    return {n[len(P):]: st.g(n).detach().cpu() for n in st.shapes if st.is_trainable(n)}


def _check_enc_grads(got, ref, dtype, what):
    """test_parity_gpu.py's bound for the tiny geometry: |got - ref| <= gtol |ref| + floor per tensor.  Its floor (1e-6 /
    2e-3) is absolute at the gradient scale of its loss, where the largest encoder gradient of the golden has norm 16.65;
    the cotangents here are arbitrary, so the floor moves with the largest gradient norm of the case."""
    gtol, floor = (2e-3, 1e-6) if dtype == F32 else (0.12, 2e-3)
    gmax = max(float(ref[k].norm()) for k in got if ref[k] is not None)
    floor *= gmax / 16.65
    worst = 0.0
    for k, v in got.items():
        r = ref[k]
        r = torch.zeros_like(v, dtype=F64) if r is None else r.to(F64)
        err, rn = float((v.to(F64).reshape(r.shape) - r).norm()), float(r.norm())
        if rn > 1e-6 * gmax:                      # (a gradient that vanishes exactly is held by the floor alone)
            worst = max(worst, err / rn)
        assert err <= gtol * rn + floor, (what, k, err, rn)
    _note(f"gpu {what} {str(dtype)[6:]}: worst encoder gradient rel err {worst:.3e} (bound {gtol:.0e}), "
          f"largest gradient norm {gmax:.3g}")


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_dmix_with_the_last_unit_vector_is_bit_equal_to_dhidden(dtype):
    from w2v2_speaker_amd.engine import Plan
    st = _enc_store(dtype)
    wav, _ = K.tiny_batch()
    plan = Plan(st, K.TINY_BATCH, K.TINY_SAMPLES, train=True, reg=_no_reg(), keep_hidden_states=True)
    D = torch.randn(K.TINY_BATCH, plan.T, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    e_L = torch.tensor([0.0, 0.0, 1.0], device=DEV)
    grads = []
    for kw in (dict(dhidden=D), dict(dmix=D, mix_weights=e_L)):
        st.grad.zero_()
        plan.forward(wav.to(DEV))
        plan.backward(**kw)
        torch.cuda.synchronize()
        grads.append(st.grad.clone())
    assert float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("variant", ["plain", "layer1-skipped", "time-mask"])
def test_dmix_encoder_gradients_against_the_float64_oracle(variant, dtype):
    from w2v2_speaker_amd.engine import Plan
    st = _enc_store(dtype)
    wav, _ = K.tiny_batch()
    ocfg, _ = K.tiny_configs()
    plan = Plan(st, K.TINY_BATCH, K.TINY_SAMPLES, train=True, reg=_no_reg(), keep_hidden_states=True)
    gen = torch.Generator().manual_seed(3)
    D = torch.randn(K.TINY_BATCH, plan.T, 64, generator=gen) / plan.T ** 0.5
    w = torch.softmax(torch.randn(3, generator=gen), 0)
    skip = (1,) if variant == "layer1-skipped" else ()
    mask = None
    if variant == "time-mask":
        mask = torch.zeros(K.TINY_BATCH, plan.T, dtype=torch.bool)
        mask[0, 2:5], mask[1, 7:9] = True, True
    st.grad.zero_()
    plan.forward(wav.to(DEV), None if mask is None else mask.to(DEV), skip)
    plan.backward(dmix=D.to(DEV), mix_weights=w.to(DEV))
    torch.cuda.synchronize()
    sd = {k: v.to(F64).clone().requires_grad_(True) for k, v in K.tiny_state()[0].items()}
    hs = K.hidden_states(wav.to(F64), sd, ocfg, skip, mask)
    sum(w[j].double() * (h * D.double()).sum() for j, h in enumerate(hs)).backward()
    _check_enc_grads(_enc_grads(st), {k: v.grad for k, v in sd.items()}, dtype, f"dmix {variant}")


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_staged_chain_every_stage_against_float64_of_its_own_input(dtype):
    from oracle import ecapa_oracle as E
    from oracle import w2v2_oracle as O
    from w2v2_speaker_amd.ecapa import FE
    from w2v2_speaker_amd.ssl_ecapa import SslEcapaPlan
    f32 = dtype == F32
    enc, ec = _enc_store(dtype), _ecapa_store(dtype)
    ocfg, ecfg = K.tiny_configs()
    sdw, sde, fcw, a = K.tiny_state()
    wav, label = K.tiny_batch()
    plan = SslEcapaPlan(enc, ec, K.TINY_BATCH, K.TINY_SAMPLES, train=True, reg=_no_reg())
    B, T, H = plan.B, plan.T, plan.H
    enc.grad.zero_()
    ec.zero_grad()
    emb = plan.embed(wav.to(DEV))
    loss, _ = plan.head_forward_backward(label.to(DEV))
    plan.backward()
    torch.cuda.synchronize()
    c = lambda t: t.detach().cpu()
    tag = str(dtype)[6:]
    # ---- hidden states (test_parity_gpu.py: 1e-4 / 3e-2)
    X = [c(x).view(B, T, H) for x in plan.enc.X]
    hs64 = K.hidden_states(wav.to(F64), {k: v.to(F64) for k, v in sdw.items()}, ocfg)
    for j, (x, h) in enumerate(zip(X, hs64)):
        assert K.rel_l2(x, h) < (1e-4 if f32 else 3e-2), j
    # ---- mix, on the GPU's own hidden states
    feat = c(plan.ecapa.feat).view(B, T, H)
    y64, r64, w64 = K.mix_forward(X, a, None, True, F64)
    y32, r32, _ = K.mix_forward(X, a, None, True, F32)
    ok, ratio, err = K.within(feat, y64, float((y32.double() - y64).abs().max()), dtype)
    _note(f"gpu staged {tag}: mix |y| err {err:.3e}, {ratio:.2f} of the bound")
    assert ok
    ok, _, _ = K.within(c(plan.rstd), r64, float((r32.double() - r64).abs().max()), F32)
    assert ok
    # ---- ECAPA forward, loss and gradients on the GPU's own features (test_ecapa_gpu.py's bounds)
    sdg = {k: v.to(F64).clone().requires_grad_(True) for k, v in sde.items()}
    fg, xg = fcw.to(F64).clone().requires_grad_(True), feat.to(F64).clone().requires_grad_(True)
    emb64 = E.ecapa_forward(xg, sdg, ecfg)
    loss64, _ = O.aam_softmax(emb64, fg, label, 0.2, 30.0)
    loss64.backward()
    loss64 = loss64.detach()
    assert K.rel_l2(c(emb), emb64.detach()) < (1e-4 if f32 else 6e-2)
    assert abs(float(loss) - float(loss64)) < (1e-4 if f32 else 5e-2) * abs(float(loss64))
    d_feat = c(plan.ecapa.d_feat)
    if f32:
        refs = {FE + k: v.grad for k, v in sdg.items()}
        refs["loss_fn.fc_weights"] = fg.grad
        gmax = max(float(v.norm()) for v in refs.values())
        for n, r in refs.items():
            err = float((c(ec.g(n)).double().reshape(r.shape) - r).norm())
            assert err <= 3e-3 * float(r.norm()) + 2e-6 * gmax, (n, err)
        assert float((d_feat.double().view(B, T, H) - xg.grad).norm()) <= 3e-3 * float(xg.grad.norm()) + 2e-6 * gmax
    # d_feat as test_ecapa_stages_gpu.py holds an inner block's data gradient: dcol from the stored da and packed weight
    # (one GEMM store), then col2im of the stored dcol (one store), each within stage_bound(r = 1)
    t0 = plan.ecapa.block0
    dcol_ref, _ = EK.tdnn_dx_ref(c(t0.da), c(t0.wp), B, T, t0.cin, t0.k, t0.dil)
    assert EK.rel_l2(c(t0.dcol), dcol_ref) <= EK.stage_bound(dcol_ref, dtype, 1)
    dfeat_ref = EK.col2im_reflect(c(t0.dcol), B, T, t0.cin, t0.k, t0.dil)
    err = EK.rel_l2(d_feat, dfeat_ref)
    _note(f"gpu staged {tag}: d_feat rel-L2 {err:.3e} (bound {EK.stage_bound(dfeat_ref, dtype, 1):.3e})")
    assert err <= EK.stage_bound(dfeat_ref, dtype, 1)
    # ---- mix backward on the GPU's own d_feat, stored y and rstd
    g3, rst = d_feat.view(B, T, H), c(plan.rstd)
    dm64, da64, _ = K.mix_backward(X, a, g3, feat, rst, True, F64)
    dm32, da32, _ = K.mix_backward(X, a, g3, feat, rst, True, F32)
    dm = c(plan.dm).view(B, T, H)
    ok, ratio, err = K.within(dm, dm64, float((dm32.double() - dm64).abs().max()), F32)
    _note(f"gpu staged {tag}: dm err {err:.3e}, {ratio:.2f} of the bound")
    assert ok
    ok, ratio, err = K.within(c(ec.g("feature_weight")), da64, float((da32.double() - da64).abs().max()), F32)
    _note(f"gpu staged {tag}: d feature_weight err {err:.3e}, {ratio:.2f} of the bound")
    assert ok
    # ---- encoder backward with the GPU's own dm and weights as the cotangent (test_parity_gpu.py's gradient bound)
    sd = {k: v.to(F64).clone().requires_grad_(True) for k, v in sdw.items()}
    hs = K.hidden_states(wav.to(F64), sd, ocfg)
    wg = c(plan.w).double()
    sum(wg[j] * (h * dm.double()).sum() for j, h in enumerate(hs)).backward()
    _check_enc_grads(_enc_grads(enc), {k: v.grad for k, v in sd.items()}, dtype, "staged encoder backward")
    if not f32:
        return
    # ---- the whole f32 chain against the composed oracle: 4 x the error of its own float32 run
    r64c, e32 = K.composed_reference()
    got = dict(loss=abs(float(loss) - float(r64c["loss"])) / abs(float(r64c["loss"])), emb=K.rel_l2(c(emb), r64c["emb"]),
               grad_a=K.rel_l2(c(ec.g("feature_weight")), r64c["grad_a"]),
               grad_fcw=K.rel_l2(c(ec.g("loss_fn.fc_weights")), r64c["grad_fcw"]),
               grads_ecapa=K.group_error({k: c(ec.g(FE + k)) for k in r64c["grads_ecapa"]}, r64c["grads_ecapa"]))
    eg = _enc_grads(enc)
    got["grads_w2v"] = K.group_error(eg, {k: v for k, v in r64c["grads_w2v"].items() if k in eg})
    for k, v in got.items():
        _note(f"gpu whole chain f32: {k} err {v:.3e} (float32 oracle {e32[k]:.3e})")
    for k, v in got.items():
        assert v <= 4 * e32[k], (k, v, e32[k])


def test_frozen_steps_leave_the_encoder_bit_unchanged_then_it_moves_and_the_loss_falls():
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.ssl_ecapa import SslEcapaPlan, SslEcapaTrainer
    enc, ec = _enc_store(F32), _ecapa_store(F32)
    B = 8
    wav, label = K.tiny_batch(B, 9)
    wav, label = wav.to(DEV), label.to(DEV)
    plan = SslEcapaPlan(enc, ec, B, K.TINY_SAMPLES, train=True, reg=_no_reg(hidden_dropout=0.1, layerdrop=0.1))
    tr = SslEcapaTrainer(plan, Constant(2e-3, 0.9), ssl_lr_factor=0.5, num_frozen_steps=2, wav2vec_initially_frozen=True)
    enc0, ec0 = enc.flat.clone(), ec.flat.clone()
    losses = [float(tr.train_step(wav, label)[0]) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(enc.flat, enc0) and enc.exp_avg is None and enc.exp_avg_sq is None and enc.step_count == 0
    fw = ec.p("feature_weight")
    assert float(fw.abs().max()) > 0 and not torch.equal(fw.cpu(), K.tiny_state()[3])
    assert not torch.equal(ec.flat, ec0)
    losses.append(float(tr.train_step(wav, label)[0]))
    torch.cuda.synchronize()
    assert not torch.equal(enc.flat, enc0) and enc.exp_avg is not None
    trainable = enc.flat[:enc.n_train] != enc0[:enc.n_train]
    assert float(trainable.float().mean()) > 0.5, "the first unfrozen step moves the encoder's trainable parameters"
    assert torch.equal(enc.flat[enc.n_train:], enc0[enc.n_train:])          # the frozen feature extractor
    losses += [float(tr.train_step(wav, label)[0]) for _ in range(7)]
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
    always = SslEcapaTrainer(plan, Constant(2e-3, 0.9), num_frozen_steps=None, wav2vec_initially_frozen=True)
    always.step = 10 ** 6
    assert always.frozen() and not SslEcapaTrainer(plan, Constant(2e-3, 0.9)).frozen()


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_variable_length_evaluation_is_bit_equal_to_each_utterance_alone(dtype):
    from w2v2_speaker_amd.ssl_ecapa import SslEcapaPlan
    enc, ec = _enc_store(dtype), _ecapa_store(dtype)
    lens = [4000, 3000, 2200]
    wav, _ = K.tiny_batch(3, 13)
    wav = wav.to(DEV)
    batch = SslEcapaPlan(enc, ec, 3, K.TINY_SAMPLES, train=False)
    emb = batch.embed(wav, lengths=lens).clone()
    hs = [h.clone() for h in batch.enc.hidden_states()]
    feat = batch.ecapa.feat.view(3, batch.T, -1).clone()
    torch.cuda.synchronize()
    assert batch.frame_lengths == batch.enc.frames_of(lens)
    for b, n in enumerate(lens):
        one = SslEcapaPlan(enc, ec, 1, n, train=False)
        e1 = one.embed(wav[b:b + 1, :n].contiguous())
        torch.cuda.synchronize()
        t = one.T
        assert t == batch.frame_lengths[b]
        for j, (hb, h1) in enumerate(zip(hs, one.enc.hidden_states())):
            assert torch.equal(hb[b, :t], h1[0]), (b, j)
        assert torch.equal(feat[b, :t], one.ecapa.feat.view(1, t, -1)[0]) and not bool(feat[b, t:].any())
        assert torch.equal(emb[b], e1[0]), b


# ---------------------------------------------------------------------------------------- module surface
def _tiny_module(dtype=F32, init_seed=20211, load=True, **cfg_kw):
    from w2v2_speaker_amd.config import W2V2Config
    from w2v2_speaker_amd.lightning_modules.speaker import Wav2vec2EcapaModule, Wav2vec2EcapaModuleConfig
    cfg = Wav2vec2EcapaModuleConfig(reset_weights=True, lin_neurons=24, channels=[64, 64, 64, 64, 192], attention_channels=16,
                                    res2net_scale=4, se_channels=16, **cfg_kw)
    tiny, orig = W2V2Config.tiny(), W2V2Config.from_huggingface_id
    W2V2Config.from_huggingface_id = staticmethod(lambda _id: tiny)          # tiny shapes behind the "base" id
    try:
        mod = Wav2vec2EcapaModule.from_config(cfg, num_speakers=K.TINY_CLASSES, device=DEV, act_dtype=dtype, ecapa_dtype=dtype,
                                              init_seed=init_seed, max_lr=2e-3, max_steps=100)
    finally:
        W2V2Config.from_huggingface_id = orig
    if load:
        sdw, sde, fcw, a = K.tiny_state()
        mod.load_state_dict({**{"wav2vec.model." + k: v for k, v in sdw.items()},
                             **{"feature_extractor." + k: v for k, v in sde.items()},
                             "loss_fn.fc_weights": fcw, "feature_weight": a}, strict=False)
    return mod


def test_module_state_dict_round_trip_gives_bit_equal_embeddings(tmp_path):
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import SpeakerClassificationDataBatch
    mod = _tiny_module(num_frozen_steps=1)
    wav, label = K.tiny_batch()
    batch = SpeakerClassificationDataBatch(wav.shape[0], [str(i) for i in range(wav.shape[0])], wav[:, None, :], label)
    enc0 = mod.enc_store.flat.clone()
    out = mod.training_step(batch)                   # frozen: BatchNorm statistics, ECAPA weights and feature_weight move
    assert torch.equal(mod.enc_store.flat, enc0) and out["loss"].numel() == 1
    mod.training_step(batch)                         # unfrozen: the encoder moves too
    torch.cuda.synchronize()
    assert not torch.equal(mod.enc_store.flat, enc0) and mod.schedule_step == 2 and mod.steps == 2
    sd = mod.state_dict()
    assert all(k.startswith(("wav2vec.model.", "feature_extractor.")) or k in ("feature_weight", "loss_fn.fc_weights")
               for k in sd), [k for k in sd][:5]
    assert "feature_weight" in sd and "feature_extractor.blocks.0.norm.norm.running_mean" in sd
    utts = [wav[0], wav[1, :3000], wav[2, :2200]]
    kw = dict(quantum=800, max_batch_samples=4 * 4000, max_batch=4)
    ref = mod.compute_speaker_embeddings(utts, **kw)
    fresh = _tiny_module(init_seed=7, load=False)
    assert not torch.equal(fresh.compute_speaker_embeddings(utts, **kw)[0], ref[0])
    fresh.load_state_dict(sd)
    for a, b in zip(fresh.compute_speaker_embeddings(utts, **kw), ref):
        assert torch.equal(a, b)
    for u, e in zip(utts, ref):                      # bucketed = each utterance alone
        assert torch.equal(mod.compute_speaker_embedding(u), e)
    assert torch.equal(mod.compute_speaker_prediction(ref[0]), ref[0].squeeze())
    path = str(tmp_path / "ssl_ecapa.ckpt")
    mod.save_checkpoint(path)
    again = _tiny_module(init_seed=9, load=False)
    again.load_checkpoint(path)
    assert again.schedule_step == 2 and torch.equal(again.compute_speaker_embeddings(utts, **kw)[1], ref[1])


def test_module_evaluate_trials_host_and_device_scoring_agree():
    import numpy as np
    import scoring_cases as SC
    from w2v2_speaker_amd.data.synthetic import synth_trial_set
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import EvaluationPair
    mod = _tiny_module()
    wav, _, keys, trials = synth_trial_set(n_speakers=4, utts_per_speaker=3, n_samples=8000)
    r = np.random.default_rng(3)
    audio = {k: torch.from_numpy(wav[i, :int(r.integers(2200, 8000))].copy()) for i, k in enumerate(keys)}
    pairs = [EvaluationPair(bool(s), keys[i], keys[j]) for s, i, j in trials]
    kw = dict(quantum=800, max_batch_samples=4 * 8000, max_batch=4)
    skeys = sorted(keys)
    idx = [(skeys.index(p.sample1_id), skeys.index(p.sample2_id)) for p in pairs]
    bank = torch.cat(mod.compute_speaker_embeddings([audio[k] for k in skeys], **kw)).cpu().numpy()
    _, score = SC.score_pairs_ref(bank, idx)
    host_score = SC.host_pairs(bank, idx)[1]
    b = SC.bound(np.abs(host_score - score).max())                     # test_scoring_gpu.py's bound
    host = mod.evaluate_trials(pairs, audio, **kw)
    dev = mod.evaluate_trials(pairs, audio, scoring="device", **kw)
    rec = mod.evaluator.last_bank_scoring
    assert np.abs(rec.scores - score).max() <= b and np.abs(rec.scores - host_score).max() <= b
    both = mod.evaluate_trials(pairs, audio, scoring="device", metrics="device", **kw)
    # scores that agree within b order the trials alike unless two of them lie closer than 2 b: then one trial may move
    gap = float(np.diff(np.sort(score)).min())
    step = 0.0 if gap > 2 * b else 1.0 / min(sum(p.same_speaker for p in pairs), sum(not p.same_speaker for p in pairs))
    _note(f"gpu module evaluate_trials: EER host {host['eer']:.4f} device {dev['eer']:.4f} device metrics {both['eer']:.4f}; "
          f"scores vs float64 {np.abs(rec.scores - score).max():.2e} (bound {b:.2e})")
    assert 0.0 <= host["eer"] <= 1.0
    assert abs(dev["eer"] - host["eer"]) <= step + 1e-9 and abs(both["eer"] - host["eer"]) <= step + 1e-9
