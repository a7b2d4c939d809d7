"""Every stage of the ECAPA-TDNN backward (w2v2_speaker_amd/ecapa.py) on the device against a float64 evaluation of the
SAME stage on the operands the plan itself stored (tests/ecapa_stage_cases.py), in f32 and bf16.

After one complete ``plan.backward()`` every intermediate still holds what its consumer read: each TDNN block owns its
a / mean_rstd / da / dcol, each SE-Res2Net block its d_se / d_t2 / d_r2 / d_t1, each SE block its s / z / g / dg / dz / ds,
and the blocks run last to first, so a slice of d_cat is final before the block that reads it as its output gradient
runs.  So the test runs the plan's own embed / head_forward_backward / backward and checks stage by stage: a 16-bit
check sees one rounding (three at the most) instead of the chain that the BatchNorm backwards amplify.

Bounds (ecapa_stage_cases.stage_bound): 2 * r * floor + 2e-5, floor = the rel-L2 distance of the reference to itself
rounded to the stored dtype (zero for f32 buffers), r = roundings to that dtype between the stored inputs and the stored
output, read from the code and written at each call.  Sums whose terms cancel (dgamma, dbeta, the SE biases) are held to
2e-5 of the sum of their |terms|.  Nothing is left out of any comparison."""
import pytest
import torch

import ecapa_stage_cases as K
from oracle import ecapa_oracle as E
from oracle import w2v2_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32


class _Report:
    """Worst figure per stage kind (printed before anything is asserted) and the list of misses."""

    def __init__(self, tag: str):
        self.tag, self.worst, self.bad = tag, {}, []

    def _note(self, kind, item, err, floor, bound):
        ratio = err / bound
        if kind not in self.worst or ratio > self.worst[kind][0]:
            self.worst[kind] = (ratio, err, floor, bound, item)
        if not err <= bound:
            self.bad.append((kind, item, err, bound))

    def stage(self, kind, item, got, ref, dtype, r):
        assert got.shape == ref.shape, (kind, item, got.shape, ref.shape)
        self._note(kind, item, K.rel_l2(got, ref), K.rounding_floor(ref, dtype), K.stage_bound(ref, dtype, r))

    def sums(self, kind, item, got, ref, sum_abs):
        assert got.shape == ref.shape == sum_abs.shape, (kind, item)
        self._note(kind + " /sum|terms|", item, K.sum_scale_error(got, ref, sum_abs), 0.0, K.F32_BOUND)

    def exact(self, kind, item, ok: bool):
        self._note(kind + " (bit-equal)", item, 0.0 if ok else float("inf"), 0.0, K.F32_BOUND)

    def flush(self):
        for kind, (_, err, floor, bound, item) in self.worst.items():
            print(f"ecapa-stage-parity: {self.tag} {kind}: worst {err:.2e} floor {floor:.2e} bound {bound:.2e} ({item})")
        missed = {}                           # kind -> (misses, the first of them: item, error, bound)
        for kind, item, err, bound in self.bad:
            missed[kind] = (missed[kind][0] + 1,) + missed[kind][1:] if kind in missed else (1, item, err, bound)
        assert not missed, (self.tag, missed)


def _make(name, dtype):
    from w2v2_speaker_amd.ecapa import EcapaConfig, EcapaPlan, EcapaStore
    kw, mels, B, T = K.GEOMETRIES[name]
    cfg = EcapaConfig(input_mel_coefficients=mels, kernel_sizes=K.KERNEL_SIZES, dilations=K.DILATIONS, **kw)
    if name == "tiny":
        assert cfg == EcapaConfig.tiny()
    st = EcapaStore(cfg, DEV, dtype, num_speakers=K.CLASSES)
    sd = E.make_state_dict(K.oracle_config(name), 20211)
    sd["loss_fn.fc_weights"] = O.synth_tensor("loss_fn.fc_weights", (K.CLASSES, cfg.lin_neurons), 20211)
    st.load_state_dict(sd)
    return cfg, st, EcapaPlan(st, B, T, train=True)


def _step(plan, st, feat, label):
    st.zero_grad()
    plan.embed(feat.to(DEV))
    plan.head_forward_backward(label.to(DEV))
    plan.backward()
    torch.cuda.synchronize()


def _snapshot(plan, st):
    """Everything the checks read, copied to the CPU once."""
    c = lambda t: None if t is None else t.detach().cpu()
    snap = {"P": {n: c(st.p(n)) for n in st.shapes}, "G": {n: c(st.g(n)) for n in st.shapes}, "tdnn": {}, "blocks": [],
            "d_cat": c(plan.d_cat), "d_x0": c(plan.d_x0), "d_mfa": c(plan.d_mfa)}
    for t in plan._tdnns():
        snap["tdnn"][t.pre] = {"a": c(t.a), "mean_rstd": c(t.mean_rstd), "da": c(t.da), "dcol": c(t.dcol), "wp": c(t.wp),
                               "wpt": c(t.wpt), "da_tail": c(t.da._full[t.M:]) if hasattr(t.da, "_full") else None}
    for b in plan.blocks:
        e = b.se
        snap["blocks"].append({"d_se": c(b.d_se), "d_t2": c(b.d_t2), "d_r2": c(b.d_r2), "d_t1": c(b.d_t1), "t2": c(b.t2),
                               "se_out": c(b.se_out), "s": c(e.s), "z": c(e.z), "g": c(e.g), "dg": c(e.dg), "dz": c(e.dz),
                               "ds": c(e.ds)})
    return snap


def _check_operands(rep, plan, snap, dtype):
    """The GEMM operand copies: wp = the f32 master packed [cout][tap][cin] and rounded to the plan's dtype; in bf16 the
    data-gradient products read wpt, which must be wp transposed -- both bit for bit."""
    for t in plan._tdnns():
        s = snap["tdnn"][t.pre]
        rep.exact("wp == pack(master)", t.pre, torch.equal(s["wp"], K.pack_conv_weight(snap["P"][t.pre + "conv.conv.weight"]).to(dtype)))
        if dtype == torch.bfloat16:
            assert s["wpt"] is not None, "the bf16 training plan keeps transposed weights"
            rep.exact("wpt == wp^T", t.pre, torch.equal(s["wpt"], s["wp"].t()))
        else:
            assert s["wpt"] is None


def _check_stages(rep, plan, snap, dtype):
    cfg, B, T = plan.cfg, plan.B, plan.T
    P, G, TD = snap["P"], snap["G"], snap["tdnn"]
    C1, nb = cfg.channels[1], len(plan.blocks)
    d_cat, d_x0 = snap["d_cat"], snap["d_x0"]

    def bn_stage(t, dy, dy2=None):
        s = TD[t.pre]
        o = K.bn_bwd_ref(s["a"], P[t.pre + "norm.norm.weight"], dy, dy2)
        rep.stage("bn mean", t.pre, s["mean_rstd"][:, 0], o["mu"], F32, 1)
        rep.stage("bn rstd", t.pre, s["mean_rstd"][:, 1], o["rstd"], F32, 1)
        # r = 1: bn_bwd adds dy + dy2 and works in f32 from the stored dy, a, mean_rstd; da is rounded at its store
        rep.stage("da" if dy2 is None else "da (dy + dy2)", t.pre, s["da"], o["da"], dtype, 1)
        rep.sums("dgamma", t.pre, G[t.pre + "norm.norm.weight"], o["dgamma"], o["dgamma_abs"])
        rep.sums("dbeta", t.pre, G[t.pre + "norm.norm.bias"], o["dbeta"], o["dbeta_abs"])
        if s["da_tail"] is not None:          # rows M .. of the row-padded storage: read by the grouped weight gradients
            rep.exact("da padding rows zero", t.pre, not bool(s["da_tail"].any()))

    def dx_of(t):
        """f64 (dcol, dx) of TDNN t from its stored da and the stored operand wp."""
        s = TD[t.pre]
        return K.tdnn_dx_ref(s["da"], s["wp"], B, T, t.cin, t.k, t.dil)

    # MFA layer (k = 1): d_cat = da @ Wp, one GEMM store; only the last slice is still that product afterwards
    bn_stage(plan.mfa, snap["d_mfa"])
    assert plan.mfa.k == 1
    mfa_dx = dx_of(plan.mfa)[1]
    rep.stage("d_cat last slice = mfa dx", "mfa.", d_cat[:, (nb - 1) * C1:], mfa_dx[:, (nb - 1) * C1:], dtype, 1)   # r = 1: GEMM store

    for i in range(nb, 0, -1):
        b, s = plan.blocks[i - 1], snap["blocks"][i - 1]
        w, sc, C = b.w, b.sc, b.C
        name = f"blocks.{i}."
        dout = d_cat[:, (i - 1) * C1:i * C1]
        rep.exact("d_se == dout slice of d_cat", name, torch.equal(s["d_se"], dout))
        # ---- SE block, forward values and backward, each from the stored operands
        e = b.se
        W1, W2 = P[e.pre + "conv1.conv.weight"][:, :, 0], P[e.pre + "conv2.conv.weight"][:, :, 0]
        x3, d3 = s["t2"].view(B, T, C), s["d_se"].view(B, T, C)
        fs, fz, fg = K.se_fwd_ref(x3, W1, P[e.pre + "conv1.conv.bias"], W2, P[e.pre + "conv2.conv.bias"])
        rep.stage("se s", name, s["s"], fs, F32, 1)
        rep.stage("se z", name, s["z"], fz, F32, 1)
        rep.stage("se g", name, s["g"], fg, F32, 1)
        rep.stage("se out", name, s["se_out"], (x3.double() * s["g"].double()[:, None]).view(B * T, C), dtype, 1)   # r = 1: se_scale store
        o = K.se_bwd_ref(x3, d3, s["s"], s["z"], s["g"], W1, W2, dg=s["dg"], dz=s["dz"], ds=s["ds"])
        rep.stage("se dg", name, s["dg"], o["dg"], F32, 1)
        rep.stage("se dz", name, s["dz"], o["dz"], F32, 1)
        rep.stage("se ds", name, s["ds"], o["ds"], F32, 1)
        rep.stage("se d_t2", name, s["d_t2"], o["d_t2"].view(B * T, C), dtype, 1)     # r = 1: se_bwd_x works in f32, one store
        rep.stage("se dW1", name, G[e.pre + "conv1.conv.weight"][:, :, 0], o["dW1"], F32, 1)
        rep.stage("se dW2", name, G[e.pre + "conv2.conv.weight"][:, :, 0], o["dW2"], F32, 1)
        rep.sums("se db1", name, G[e.pre + "conv1.conv.bias"], o["db1"], o["db1_abs"])
        rep.sums("se db2", name, G[e.pre + "conv2.conv.bias"], o["db2"], o["db2_abs"])
        # ---- tdnn2 (k = 1): d_r2 = da @ Wp
        bn_stage(b.tdnn2, s["d_t2"])
        rep.stage("d_r2 = tdnn2 dx", name, s["d_r2"], dx_of(b.tdnn2)[1], dtype, 1)     # r = 1: GEMM store
        # ---- Res2Net chunks, last first: chunk j < sc - 1 also feeds chunk j + 1
        for j in range(sc - 1, 0, -1):
            t = b.chunks[j]
            dy2 = s["d_t1"][:, (j + 1) * w:(j + 2) * w] if j < sc - 1 else None
            bn_stage(t, s["d_r2"][:, j * w:(j + 1) * w], dy2)
            assert t.k > 1
            dcol_ref = dx_of(t)[0]
            rep.stage("dcol", t.pre, TD[t.pre]["dcol"], dcol_ref, dtype, 1)             # r = 1: GEMM store
            # from the STORED dcol; r = 1: col2im_reflect sums its taps in f32 and stores once
            rep.stage("d_t1 slice = col2im(dcol)", t.pre, s["d_t1"][:, j * w:(j + 1) * w],
                      K.col2im_reflect(TD[t.pre]["dcol"], B, T, w, t.k, t.dil), dtype, 1)
        rep.exact("d_t1[:, :w] == d_r2[:, :w]", name, torch.equal(s["d_t1"][:, :w], s["d_r2"][:, :w]))
        # ---- tdnn1 (k = 1) and the residual
        bn_stage(b.tdnn1, s["d_t1"])
        dx1 = dx_of(b.tdnn1)[1]
        if i == 1:      # r = 2: the GEMM stores da @ Wp, the residual add_strided rounds the sum
            rep.stage("d_x0 = tdnn1 dx + dout", name, d_x0, dx1 + dout.double(), dtype, 2)
        else:           # r = 3: the MFA GEMM's store, the EPI_ADD GEMM onto it, the residual add_strided
            sl = slice((i - 2) * C1, (i - 1) * C1)
            rep.stage("d_cat slice = mfa dx + tdnn1 dx + dout", name, d_cat[:, sl], mfa_dx[:, sl] + dx1 + dout.double(), dtype, 3)
    bn_stage(plan.block0, d_x0)               # (the features need no gradient: block 0 has no data-gradient product)


@pytest.mark.parametrize("name", ["tiny", "narrow"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_every_ecapa_backward_stage_vs_f64_of_its_stored_operands(dtype, name):
    """One training step, every stage; then an optimiser step and a second forward / backward on another input, where a
    stale or mis-strided operand copy (wp, and wpt of the bf16 data-gradient products) would show."""
    cfg, st, plan = _make(name, dtype)
    tag = f"{name} {'f32' if dtype == F32 else 'bf16'}"
    _step(plan, st, *K.inputs(name, 3))
    snap1 = _snapshot(plan, st)
    rep = _Report(tag + " step 1")
    _check_operands(rep, plan, snap1, dtype)
    _check_stages(rep, plan, snap1, dtype)
    rep.flush()

    st.optimizer_step(lr=1e-2)
    _step(plan, st, *K.inputs(name, 4))
    snap2 = _snapshot(plan, st)
    rep = _Report(tag + " step 2")
    for t in plan._tdnns():                   # the update is no no-op: every operand copy has to have moved
        rep.exact("wp moved with the optimiser step", t.pre, not torch.equal(snap1["tdnn"][t.pre]["wp"], snap2["tdnn"][t.pre]["wp"]))
    _check_operands(rep, plan, snap2, dtype)
    _check_stages(rep, plan, snap2, dtype)
    rep.flush()
