"""The x-vector path on the device (w2v2_speaker_amd/xvector.py, csrc/tdnn.hip): the new kernels against float64 of their
stored operands, two whole training steps stage by stage against the float64 restatement of tests/xvector_cases.py, and
the evaluation contract (a row of a padded batch is the utterance alone, bit for bit).

Bounds: every stage is f32 from stored f32 operands, so the bound of the project's ECAPA stage tests applies with a
rounding floor of zero: 2e-5 rel-L2 (ecapa_stage_cases.F32_BOUND); sums whose terms cancel (dgamma, dbeta, the bias
gradients) are held to 2e-5 of the sum of their |terms|.  The worst figure per stage kind is printed before anything is
asserted (``pytest -s``; profiles/xvector_parity.txt)."""
import pytest
import torch
import torch.nn.functional as F

import xvector_cases as K
from w2v2_speaker_amd import ops
from w2v2_speaker_amd import xvector as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
BOUND = K.F32_BOUND


class _Report:
    """Worst figure per stage kind (printed before anything is asserted) and the list of misses."""

    def __init__(self, tag: str):
        self.tag, self.worst, self.bad = tag, {}, []

    def note(self, kind, item, err):
        if kind not in self.worst or err > self.worst[kind][0] or err != err:
            self.worst[kind] = (err, item)
        if not err <= BOUND:
            self.bad.append((kind, item, err))

    def stage(self, kind, item, got, ref):
        assert got.shape == ref.shape, (kind, item, got.shape, ref.shape)
        self.note(kind, item, K.rel_l2(got, ref))

    def sums(self, kind, item, got, ref, sum_abs):
        assert got.shape == ref.shape == sum_abs.shape, (kind, item)
        self.note(kind + " /sum|terms|", item, K.sum_scale_error(got, ref, sum_abs))

    def flush(self):
        for kind, (err, item) in self.worst.items():
            print(f"xvector-parity: {self.tag} {kind}: worst {err:.2e} bound {BOUND:.2e} ({item})")
        assert not self.bad, (self.tag, self.bad[:6], len(self.bad))


def _cpu(t):
    return None if t is None else t.detach().cpu()


# ------------------------------------------------------------------------------------------------ LeakyReLU -> BatchNorm
def _bn_input(M, C, ld, kind):
    g = torch.Generator().manual_seed(1000 * M + C)
    a = torch.randn(M, ld, generator=g) * 1.5 + 0.3
    if kind == "zeros":            # exact zeros (the backward's slope at a == 0) and a majority of negative values
        a = a - 1.5
        a[torch.rand(M, ld, generator=g) < 0.25] = 0.0
    return a, torch.randn(M, ld, generator=g), torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)


@pytest.mark.parametrize("kind", ["randn", "zeros"])
@pytest.mark.parametrize("M", K.BN_ROWS)
def test_leaky_relu_batchnorm_kernels_vs_float64(M, kind):
    rep = _Report(f"leaky-bn M={M} {kind}")
    for C, ld in [(K.BN_CHANNELS[0], K.BN_CHANNELS[0] + 4), (K.BN_CHANNELS[1], K.BN_CHANNELS[1])]:
        a, dy, gamma, beta = _bn_input(M, C, ld, kind)
        if kind == "zeros":
            assert int((a[:, :C] == 0).sum()) > 0 and int((a[:, :C] < 0).sum()) > a[:, :C].numel() // 2
        ad, dyd, gd, bd = a.to(DEV), dy.to(DEV), gamma.to(DEV), beta.to(DEV)
        y, da = torch.full((M, ld), 7.0, device=DEV), torch.full((M, ld), 7.0, device=DEV)
        work, mr = ops.bn_workspace(M, C, DEV), torch.empty(C, 2, device=DEV)
        run0 = torch.cat([torch.randn(C), torch.rand(C) + 0.5])
        running = run0.to(DEV)
        ops.bn_fwd(ad, ld, work, mr, running, gd, bd, y, ld, M, C, K.BN_EPS, K.BN_MOMENTUM, ops.BN_ACT_LEAKY, True)
        f = K.act_bn_fwd_ref(a[:, :C], gamma, beta)
        item = f"C={C} ld={ld}"
        mrc = _cpu(mr)
        # the statistics: the mean, and the variance as the cancelling sum E[r^2] - mean^2 that it is (over two rows a
        # channel's two values may agree to several digits); then the normalisation with the statistics it used
        rep.stage("mean", item, mrc[:, 0], f["mu"])
        rep.stage("y (stored statistics)", item, _cpu(y)[:, :C], K.act_bn_apply_ref(a[:, :C], gamma, beta, mrc))
        if M >= 255:
            rep.stage("y (float64 chain)", item, _cpu(y)[:, :C], f["y"])
            rep.stage("rstd", item, mrc[:, 1], f["rstd"])
        rep.note("var + eps = 1 / rstd^2 /sum|terms|", item, K.variance_error(mrc, a[:, :C]))
        rm, rv = K.running_ref(run0[:C], run0[C:], f["mu"], f["var"], M)
        rep.stage("running_mean", item, _cpu(running)[:C], rm)
        rep.stage("running_var", item, _cpu(running)[C:], rv)
        dgam, dbet = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        csp = torch.full((ops.bn_colsum_rows(M, C), C), float("nan"), device=DEV)
        ops.bn_bwd(dyd, ld, ad, ld, mr, gd, work, dgam, dbet, da, ld, M, C, ops.BN_ACT_LEAKY, colsum_partial=csp)
        # the backward reads the STORED statistics: float64 from those.  da is a difference of three terms that cancels
        # almost entirely over two rows (it is exactly 0 without the eps), so it is held to the sum of their magnitudes;
        # where the rows are many it must also agree with the float64 chain as a whole
        o = K.act_bn_bwd_ref(a[:, :C], gamma, dy[:, :C], stats=(mrc[:, 0], mrc[:, 1]))
        dac = _cpu(da)[:, :C]
        rep.sums("da", item, dac, o["da"], o["da_abs"])
        if M >= 255:
            rep.stage("da (float64 chain)", item, dac, K.act_bn_bwd_ref(a[:, :C], gamma, dy[:, :C])["da"])
        rep.sums("dgamma", item, _cpu(dgam), o["dgamma"], o["dgamma_abs"])
        rep.sums("dbeta", item, _cpu(dbet), o["dbeta"], o["dbeta_abs"])
        rep.sums("colsum(da)", item, _cpu(csp).double().sum(0), dac.double().sum(0), dac.double().abs().sum(0))
        if ld > C:                     # columns outside the view: untouched by both directions
            assert bool((_cpu(y)[:, C:] == 7.0).all()) and bool((_cpu(da)[:, C:] == 7.0).all())
        # evaluation: the running statistics, which stay as they are
        run1 = running.clone()
        ops.bn_fwd(ad, ld, None, mr, running, gd, bd, y, ld, M, C, K.BN_EPS, K.BN_MOMENTUM, ops.BN_ACT_LEAKY, False)
        rep.stage("y (eval)", item, _cpu(y)[:, :C], K.act_bn_eval_ref(a[:, :C], gamma, beta, _cpu(run1)[:C], _cpu(run1)[C:]))
        assert torch.equal(running, run1)
    rep.flush()


def test_batchnorm_rejects_an_unknown_activation_and_f32_takes_multiples_of_four():
    M, C = 8, 12
    a = torch.randn(M, C, device=DEV)
    y, mr, work = torch.empty_like(a), torch.empty(C, 2, device=DEV), ops.bn_workspace(M, C, DEV)
    g, b = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    for act in (ops.BN_ACT_NONE, ops.BN_ACT_RELU, ops.BN_ACT_LEAKY):
        ops.bn_fwd(a, C, work, mr, None, g, b, y, C, M, C, K.BN_EPS, K.BN_MOMENTUM, act, True)
    with pytest.raises(RuntimeError):
        ops.bn_fwd(a, C, work, mr, None, g, b, y, C, M, C, K.BN_EPS, K.BN_MOMENTUM, 3, True)
    with pytest.raises(RuntimeError):                     # a 16-bit tensor still needs whole 8-channel vectors
        ops.bn_fwd(a.bfloat16(), C, work, mr, None, g, b, y.bfloat16(), C, M, C, K.BN_EPS, K.BN_MOMENTUM, 2, True)


# ------------------------------------------------------------------------------------------------ statistics pooling
@pytest.mark.parametrize("T", K.POOL_FRAMES)
def test_statistics_pool_forward_backward_and_lengths_vs_float64(T):
    B, C, ld = 3, K.POOL_C, K.POOL_LD
    g = torch.Generator().manual_seed(T)
    x = torch.randn(B, T, ld, generator=g) + 0.5
    x[:, :, C:] = 3.0                                       # constant columns next to the pooled range: never read
    dout = torch.randn(B, 2 * C, generator=g)
    xd = x.to(DEV).view(B * T, ld)
    out, stats = torch.empty(B, 2 * C, device=DEV), torch.empty(B, 2 * C, device=DEV)
    ops.stat_pool_fwd(xd, ld, out, stats, B, T, C)
    mean, std, ref = K.stat_pool_fwd_ref(x[:, :, :C])
    rep = _Report(f"stat-pool T={T}")
    rep.stage("out = cat(mean, std + eps)", "", _cpu(out), ref)
    rep.stage("stats mean", "", _cpu(stats)[:, :C], mean)
    rep.stage("stats std", "", _cpu(stats)[:, C:], std)
    assert torch.equal(out[:, :C], stats[:, :C])            # the mean comes first
    dx = torch.full((B * T, ld), 7.0, device=DEV)
    ops.stat_pool_bwd(xd, ld, stats, dout.to(DEV), dx, ld, B, T, C)
    dxc = _cpu(dx).view(B, T, ld)
    # from the STORED statistics, as the kernel reads them
    s64 = _cpu(stats).double()
    want = dout.double()[:, None, :C] / T + dout.double()[:, None, C:] * (x[:, :, :C].double() - s64[:, None, :C]) / (
        (T - 1) * s64[:, None, C:])
    rep.stage("dx (stored stats)", "", dxc[:, :, :C], want)
    rep.stage("dx (float64 chain)", "", dxc[:, :, :C], K.stat_pool_bwd_ref(x[:, :, :C], dout))
    assert bool(torch.isfinite(dxc).all()) and bool((dxc[:, :, C:] == 7.0).all())       # no NaN, padding columns untouched
    if T >= 5:                  # (T = 2 has no shorter valid length: the unbiased std needs two frames, the model four)
        lens = [T, T - 1, 4]
        noisy = x.clone()
        for b, n in enumerate(lens):
            noisy[b, n:] = 1e3 * torch.randn(T - n, ld, generator=g)
        out_l = torch.empty(B, 2 * C, device=DEV)
        ops.stat_pool_fwd(noisy.to(DEV).view(B * T, ld), ld, out_l, None, B, T, C,
                          lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
        rep.stage("out (lengths)", str(lens), _cpu(out_l), K.stat_pool_fwd_ref(x[:, :, :C], lens)[2])
        for b, n in enumerate(lens):
            alone = torch.empty(1, 2 * C, device=DEV)
            ops.stat_pool_fwd(x[b, :n].contiguous().to(DEV), ld, alone, None, 1, n, C)
            assert torch.equal(out_l[b:b + 1], alone), (b, n)
    rep.flush()


def test_statistics_pool_constant_column_has_torchs_gradient_and_no_nan():
    """std = 0 in a constant column: torch's std backward masks the 0 / 0 there, so the column gets dmean / T only."""
    B, T, C = 2, 9, 8
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(3))
    x[:, :, 5] = 1.25
    xr = x.double().requires_grad_()
    std, mean = torch.std_mean(xr, dim=1)
    dout = torch.randn(B, 2 * C, generator=torch.Generator().manual_seed(4))
    (torch.cat([mean, std], 1) * dout.double()).sum().backward()
    out, stats, dx = (torch.empty(B, 2 * C, device=DEV), torch.empty(B, 2 * C, device=DEV), torch.empty(B * T, C, device=DEV))
    xd = x.to(DEV).view(B * T, C)
    ops.stat_pool_fwd(xd, C, out, stats, B, T, C)
    assert bool((_cpu(stats)[:, C + 5] == 0).all()) and bool((_cpu(out)[:, C + 5] == K.POOL_EPS).all())
    ops.stat_pool_bwd(xd, C, stats, dout.to(DEV), dx, C, B, T, C)
    got = _cpu(dx).view(B, T, C)
    assert bool(torch.isfinite(xr.grad).all()) and bool(torch.isfinite(got).all())
    assert K.rel_l2(got[:, :, 5], xr.grad[:, :, 5]) <= BOUND and K.rel_l2(got, xr.grad) <= BOUND
    assert K.rel_l2(K.stat_pool_bwd_ref(x, dout), xr.grad) <= 1e-12


# ------------------------------------------------------------------------------------------------ the whole model
def _store(seed=20211, cfg=None, speakers=K.SPEAKERS):
    cfg = cfg or X.XVectorConfig.tiny()
    st = X.XVectorStore(cfg, DEV, num_speakers=speakers)
    st.load_state_dict(K.make_state_dict(seed, mels=cfg.input_mel_coefficients, channels=cfg.channels,
                                         kernel_sizes=cfg.kernel_sizes, lin=cfg.lin_neurons, speakers=speakers))
    return st


def _moved_running(st, seed=5):
    """Running statistics away from (0, 1), as after training."""
    g = torch.Generator().manual_seed(seed)
    for r in st.bn_running.values():
        C = r.numel() // 2
        r.copy_(torch.cat([0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)]).to(DEV))
    return st


def _snapshot(plan, st, P):
    cl, h = plan.classifier, plan.classifier.head
    snap = {"P": P, "G": {n: _cpu(st.g(n)) for n in st.shapes}, "feat": _cpu(plan.feat), "tdnn": [],
            "pooled": _cpu(plan.pooled), "stats": _cpu(plan.pool_stats), "emb": _cpu(plan.emb), "dpooled": _cpu(plan.linear.dx),
            "z": _cpu(cl.z), "dh1": _cpu(cl.dnn.dx), "logits": _cpu(h.logits)[:, :h.C], "softmax": _cpu(h.softmax)[:, :h.C],
            "dlogits": _cpu(h.dcos_w)[:, :h.C], "dh2": _cpu(h.demb), "d_x": [_cpu(t) for t in plan.d_x]}
    for t in plan.tdnns:
        snap["tdnn"].append({"a": _cpu(t.a), "mean_rstd": _cpu(t.mean_rstd), "y": _cpu(t.y), "da": _cpu(t.da),
                             "wp": _cpu(t.wp)})
    for name, n in (("norm1", cl.norm1), ("norm2", cl.norm2)):
        snap[name] = {"a": _cpu(n.a), "y": _cpu(n.y), "mean_rstd": _cpu(n.mean_rstd), "da": _cpu(n.da)}
    return snap


def _check_stages(rep, plan, snap, loss, label):
    """Every stage against float64 of the operands the plan stored for that stage."""
    P, G, cfg, B, T = snap["P"], snap["G"], plan.cfg, plan.B, plan.T

    def act_bn(kind, item, s, gname, bname, dy, dbias_name):
        """The statistics (the variance as the cancelling sum it is), the normalisation with the statistics it used, and
        the backward from the stored statistics it reads; over the B * T rows of a TDNN block also the float64 chain."""
        mr, M = s["mean_rstd"], s["a"].shape[0]
        f = K.act_bn_fwd_ref(s["a"], P[gname], P[bname])
        rep.stage(kind + " mean", item, mr[:, 0], f["mu"])
        rep.note(kind + " var + eps = 1 / rstd^2 /sum|terms|", item, K.variance_error(mr, s["a"]))
        rep.stage(kind + " y", item, s["y"], K.act_bn_apply_ref(s["a"], P[gname], P[bname], mr))
        o = K.act_bn_bwd_ref(s["a"], P[gname], dy, stats=(mr[:, 0], mr[:, 1]))
        rep.stage(kind + " da", item, s["da"], o["da"])
        if M >= 255:
            rep.stage(kind + " rstd", item, mr[:, 1], f["rstd"])
            rep.stage(kind + " y (float64 chain)", item, s["y"], f["y"])
            rep.stage(kind + " da (float64 chain)", item, s["da"], K.act_bn_bwd_ref(s["a"], P[gname], dy)["da"])
        rep.sums(kind + " dgamma", item, G[gname], o["dgamma"], o["dgamma_abs"])
        rep.sums(kind + " dbeta", item, G[bname], o["dbeta"], o["dbeta_abs"])
        rep.sums("bias gradient = colsum(da)", dbias_name, G[dbias_name], s["da"].double().sum(0), s["da"].double().abs().sum(0))

    def linear(kind, name, x, y, dy, dx):
        W, b = P[name + "weight"], P[name + "bias"]
        rep.stage(kind + " y", name, y, K.linear_fwd_ref(x, W, b))
        dW, _, dxr, _ = K.linear_bwd_ref(x, W, dy)
        rep.stage(kind + " dW", name, G[name + "weight"], dW)
        rep.stage(kind + " dx", name, dx, dxr)

    x = snap["feat"]
    for i, (t, s) in enumerate(zip(plan.tdnns, snap["tdnn"])):
        item = f"blocks.{3 * i}"
        W, b = P[t.n_w], P[t.n_b]
        assert torch.equal(s["wp"], K.pack_conv_weight(W)), item                       # the operand copy is the master, packed
        rep.stage("conv a", item, s["a"], K.conv_fwd_ref(x, W, b, B, T, t.k, t.dil))
        act_bn("tdnn bn", item, s, t.n_gamma, t.n_beta, snap["d_x"][i], t.n_b)
        dW, _, dx = K.conv_bwd_ref(x, W, s["da"], B, T, t.k, t.dil)
        rep.stage("conv dW", item, G[t.n_w], dW)
        if i > 0:
            rep.stage("conv dx", item, snap["d_x"][i - 1], dx)
        x = s["y"]
    CL = cfg.channels[-1]
    mean, std, pooled = K.stat_pool_fwd_ref(x.view(B, T, CL))
    rep.stage("pool out", "", snap["pooled"], pooled)
    rep.stage("pool stats", "", snap["stats"], torch.cat([mean, std], 1))
    rep.stage("pool dx", "", snap["d_x"][-1], K.stat_pool_bwd_ref(x.view(B, T, CL), snap["dpooled"]).reshape(B * T, CL))
    lin = plan.linear.n_w[:-len("weight")]
    linear("embedding linear", lin, snap["pooled"], snap["emb"], snap["norm1"]["da"], snap["dpooled"])
    act_bn("classifier bn", "norm", snap["norm1"], K.CLS + "norm.norm.weight", K.CLS + "norm.norm.bias", snap["dh1"],
           lin + "bias")
    assert torch.equal(snap["norm1"]["a"], snap["emb"]) and torch.equal(snap["norm2"]["a"], snap["z"])
    dnn = K.CLS + "DNN.block_0.linear.w."
    linear("classifier linear", dnn, snap["norm1"]["y"], snap["z"], snap["norm2"]["da"], snap["dh1"])
    act_bn("classifier bn", "DNN.block_0.norm", snap["norm2"], K.CLS + "DNN.block_0.norm.norm.weight",
           K.CLS + "DNN.block_0.norm.norm.bias", snap["dh2"], dnn + "bias")
    out = K.CLS + "out.w."
    linear("output linear", out, snap["norm2"]["y"], snap["logits"], snap["dlogits"], snap["dh2"])
    rep.sums("bias gradient = colsum(da)", out + "bias", G[out + "bias"], snap["dlogits"].double().sum(0),
             snap["dlogits"].double().abs().sum(0))
    # loss and softmax against F.cross_entropy of the restated logits (float64 from the stored classifier output)
    z = K.linear_fwd_ref(snap["norm2"]["y"], P[out + "weight"], P[out + "bias"]).requires_grad_()
    ce = F.cross_entropy(z, label)
    ce.backward()
    rep.stage("loss", "", torch.tensor([float(loss)]), ce.detach().view(1))
    rep.stage("softmax", "", snap["softmax"], torch.softmax(z.detach(), 1))
    rep.stage("dlogits", "", snap["dlogits"], z.grad)
    # ... and the reference's own form, the loss of the log-probabilities, is the same number
    assert abs(float(F.cross_entropy(torch.log_softmax(z.detach(), 1), label)) - float(ce.detach())) < 1e-12


def test_two_train_steps_every_stage_vs_float64_of_its_stored_operands():
    from w2v2_speaker_amd.optim.schedule import Constant
    st = _store()
    plan = X.XVectorPlan(st, K.B, K.T, train=True)
    tr = X.XVectorTrainer(st, plan, Constant(1e-2, 0.9))
    flats = []
    for step, seed in enumerate((3, 4)):
        feat, label = K.inputs(seed)
        P = {n: _cpu(st.p(n)).clone() for n in st.shapes}            # the parameters this step's forward and backward read
        flats.append(st.flat.clone())
        loss, softmax = tr.train_step(feat.to(DEV), label.to(DEV))
        torch.cuda.synchronize()
        assert softmax.shape == (K.B, K.SPEAKERS) and tr.stepped
        rep = _Report(f"tiny f32 step {step + 1}")
        _check_stages(rep, plan, _snapshot(plan, st, P), loss, label)
        rep.flush()
    assert not torch.equal(flats[0], flats[1]) and not torch.equal(flats[1], st.flat)      # both optimiser steps moved the arena
    # the whole chain against the float64 restatement end to end (step 2's parameters): looser by the depth of the chain
    rec = K.forward_ref(P, feat, label)
    G = K.backward_ref(P, rec)
    worst = max(K.rel_l2(_cpu(st.g(n)), G[n]) for n in st.shapes if not n.endswith("bias"))
    print(f"xvector-parity: tiny f32 step 2 end to end: loss {float(loss):.6f} vs {float(rec['loss']):.6f}, worst weight-gradient "
          f"rel-L2 vs the float64 chain {worst:.2e}")
    assert abs(float(loss) - float(rec["loss"])) <= 1e-4 * abs(float(rec["loss"]))


def test_loss_of_twenty_steps_on_a_fixed_batch_decreases():
    from w2v2_speaker_amd.optim.schedule import Constant
    st = _store()
    tr = X.XVectorTrainer(st, X.XVectorPlan(st, K.B, K.T, train=True), Constant(1e-2, 0.9))
    feat, label = K.inputs(7)
    feat, label = feat.to(DEV), label.to(DEV)
    losses = [float(tr.train_step(feat, label)[0]) for _ in range(20)]
    print(f"xvector-parity: fixed batch, 20 Adam steps: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert all(l == l for l in losses) and losses[-1] < losses[0]
    assert losses[-1] < 0.5 * losses[0]                              # three utterances, seven classes: memorised quickly


# ------------------------------------------------------------------------------------------------ evaluation
def test_bucketed_batch_rows_are_bit_identical_to_the_utterance_alone():
    st = _moved_running(_store())
    lens = [100, 57, 4]
    T = max(lens)
    g = torch.Generator().manual_seed(9)
    utts = [torch.randn(n, K.MELS, generator=g) for n in lens]
    feat = 1e3 * torch.randn(len(lens), T, K.MELS, generator=g)         # the padding holds large finite values
    for b, u in enumerate(utts):
        feat[b, :u.shape[0]] = u
    plan = X.XVectorPlan(st, len(lens), T, train=False)
    e = plan.embed(feat.to(DEV), lengths=lens).clone()
    assert plan.frame_lengths == lens and bool(torch.isfinite(e).all())
    assert torch.equal(plan.embed(feat.to(DEV), lengths=torch.tensor(lens)), e)
    for b, u in enumerate(utts):
        alone = X.XVectorPlan(st, 1, u.shape[0], train=False).embed(u[None].to(DEV))
        assert torch.equal(e[b:b + 1], alone), (b, u.shape[0])
    with pytest.raises(ValueError):
        plan.embed(feat.to(DEV), lengths=[100, 57, 3])                  # the widest reflect padding is 3 frames
    with pytest.raises(NotImplementedError):
        X.XVectorPlan(st, 3, T, train=True).embed(feat.to(DEV), lengths=lens)
    # the evaluation forward against float64 on the running statistics
    sd = {n: v.double() for n, v in st.state_dict().items() if v.is_floating_point()}
    x = utts[1].double()
    for i, (k, d) in enumerate(zip(K.KERNEL_SIZES, K.DILATIONS)):
        c, n = f"{K.FE}blocks.{3 * i}.conv.", f"{K.FE}blocks.{3 * i + 2}.norm."
        a = K.conv_fwd_ref(x, sd[c + "weight"], sd[c + "bias"], 1, lens[1], k, d)
        x = K.act_bn_eval_ref(a, sd[n + "weight"], sd[n + "bias"], sd[n + "running_mean"], sd[n + "running_var"])
    ref = K.linear_fwd_ref(K.stat_pool_fwd_ref(x[None])[2], sd[K.FE + "blocks.16.w.weight"], sd[K.FE + "blocks.16.w.bias"])
    err = K.rel_l2(_cpu(e)[1:2], ref)
    print(f"xvector-parity: evaluation embedding of a 57-frame row vs float64: rel-L2 {err:.2e}")
    assert err <= 5 * BOUND              # five chained f32 blocks, each inside the stage bound


def _module(**kw):
    from w2v2_speaker_amd.lightning_modules.speaker import XVectorModule, XVectorModuleConfig
    cfg = XVectorModuleConfig(tdnn_channels=list(K.CHANNELS), lin_neurons=K.LIN, in_channels=kw.pop("mels", K.MELS))
    mod = XVectorModule.from_config(cfg, K.SPEAKERS, **kw)
    mod.load_state_dict(K.make_state_dict(20211, mels=cfg.in_channels), strict=False)
    _moved_running(mod.store)
    return mod


def test_waveform_input_equals_fbank_input_of_the_host_features():
    import test_fbank_gpu as FB
    cfg = X.XVectorConfig(40, K.LIN, K.CHANNELS, K.KERNEL_SIZES, K.DILATIONS)
    st = _moved_running(_store(cfg=cfg))
    Bn, N = 3, 8000
    plan = X.XVectorPlan(st, Bn, X.fbank_frames(N), train=False)
    wav = FB._wavs(Bn, N)
    fb = FB._fb()
    host = torch.stack([FB._host_f32_stages(w, fb)[1] for w in wav])
    f64 = torch.stack([FB._f64_stages(w, fb)[2] for w in wav]).float()
    e_host = plan.embed(host.to(DEV)).cpu().clone()
    e_f64 = plan.embed(f64.to(DEV)).cpu().clone()
    e_dev = plan.embed_waveform(wav.to(DEV)).cpu().clone()
    bound = FB.FACTOR * FB.rel_l2(e_host, e_f64)
    err = FB.rel_l2(e_dev, e_host)
    print(f"xvector-parity: embed_waveform vs embed(host features) rel-L2 {err:.3e}; embed(host f32 features) vs "
          f"embed(float64 features) rel-L2 {bound / FB.FACTOR:.3e} (bound x{FB.FACTOR:.0f})")
    assert bound > 0 and err <= bound, (err, bound)
    # the variable-length waveform form: a row is the utterance alone
    lens = [8000, 480, 801]
    e = plan.embed_waveform(wav.to(DEV), lengths=lens).clone()
    for b, n in enumerate(lens):
        alone = X.XVectorPlan(st, 1, X.fbank_frames(n), train=False).embed_waveform(wav[b:b + 1, :n].contiguous().to(DEV))
        assert torch.equal(e[b:b + 1], alone), (b, n)


def test_module_training_step_prediction_and_trials():
    from w2v2_speaker_amd.data.synthetic import synth_trial_set
    from w2v2_speaker_amd.evaluation.speaker.cosine_distance import EvaluationPair
    from w2v2_speaker_amd.lightning_modules.speaker.wav2vec2_fc import SpeakerClassificationDataBatch
    mod = _module(max_lr=1e-2, max_steps=100, gradient_clip_val=1.0)
    assert mod.generate_example_input(True, 2).shape == (2, 100, K.MELS)
    feat, label = K.inputs(21)
    e = mod.compute_speaker_embedding(feat)
    assert e.shape == (K.B, K.LIN) and torch.equal(mod.compute_speaker_embedding(feat[0]), e[:1])
    # the prediction is the classifier's log-probabilities on the running statistics
    logp = mod.compute_speaker_prediction(e)
    sd = {n: v.double() for n, v in mod.state_dict().items() if v.is_floating_point()}
    c = K.CLS
    h = K.act_bn_eval_ref(_cpu(e), sd[c + "norm.norm.weight"], sd[c + "norm.norm.bias"], sd[c + "norm.norm.running_mean"],
                          sd[c + "norm.norm.running_var"])
    z = K.linear_fwd_ref(h, sd[c + "DNN.block_0.linear.w.weight"], sd[c + "DNN.block_0.linear.w.bias"])
    n = c + "DNN.block_0.norm.norm."
    h = K.act_bn_eval_ref(z, sd[n + "weight"], sd[n + "bias"], sd[n + "running_mean"], sd[n + "running_var"])
    ref = torch.log_softmax(K.linear_fwd_ref(h, sd[c + "out.w.weight"], sd[c + "out.w.bias"]), 1)
    assert logp.shape == (K.B, K.SPEAKERS) and K.rel_l2(_cpu(logp), ref) <= 3 * BOUND      # three chained f32 stages
    # training through the module: the optimiser surface of the other speaker modules
    mod.set_optimizer(torch.optim.SGD(mod.parameters(), lr=1e-2, momentum=0.9))
    batch = SpeakerClassificationDataBatch(K.B, [f"u{i}" for i in range(K.B)], feat, label)
    before = mod.store.flat.clone()
    out = mod.training_step(batch)
    assert out["prediction"].shape == (K.B, K.SPEAKERS) and float(out["loss"]) > 0 and mod.schedule_step == 1
    assert not torch.equal(before, mod.store.flat)
    acc = _module(accumulate_grad_batches=2)
    acc.training_step(batch)
    assert acc.schedule_step == 0 and acc.steps == 1
    acc.training_step(batch)
    assert acc.schedule_step == 1 and acc.steps == 2
    # trials
    wav, _, keys, trials = synth_trial_set(n_speakers=3, utts_per_speaker=2, n_samples=1600, seed=4)
    g = torch.Generator().manual_seed(2)
    feats = {k: torch.randn(int(torch.randint(4, 60, (1,), generator=g)), K.MELS, generator=g) for k in keys}
    pairs = [EvaluationPair(bool(s), keys[i], keys[j]) for s, i, j in trials]
    ev = _module()
    got = ev.evaluate_trials(pairs, feats, quantum=10, max_batch_frames=120, max_batch=4)
    assert isinstance(got, dict) and "eer" in got and 0.0 <= got["eer"] <= 1.0
    embs = ev.compute_speaker_embeddings([feats[k] for k in keys], quantum=10, max_batch_frames=120, max_batch=4)
    for k, eb in zip(keys, embs):
        assert torch.equal(eb, ev.compute_speaker_embedding(feats[k])), k
