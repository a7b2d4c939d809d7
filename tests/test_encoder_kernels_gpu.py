"""GPU tests of csrc/norm.hip (w2v2_layernorm_fwd / _bwd / _bwd_fold) and csrc/attention.hip (w2v2_attention_fwd / _bwd)
against the float64 references of tests/encoder_cases.py, at the edges where these kernels can go wrong.

Layer norm: one lane / an empty or one-lane second chunk / both quad widths / both chunks full; fewer rows than a workgroup
has waves; 2 * 4 * cap + 5 rows, where a wave walks two or three rows (grid stride, next-row prefetch in the middle and at
its end, column sums over several rows); all three backward kernels through dtype, H and the dgamma argument; rows with a DC
component, with outliers and with zero variance.  Attention: every T around a 16-row fragment, a 32- and a 64-row tile and
the geometry threshold under both geometries, with and without LDS-DMA tile loads; scores that are uniform, that put the
maximum on the last or the first key, that are one-hot, that overflow without the maximum subtracted; gradients below fp16's
normal range; dropout masks read back from each of the three kernels.

Every output is judged per row (and per column where a column is a reduction), between sentinel rows, out of a pre-filled
buffer; every backward runs twice and must repeat itself bit for bit.  Each backward is tested on inputs computed by the
float64 reference, so a forward failure cannot show as a backward failure; one chained test per family feeds the device
forward's outputs into the device backward.  Every test prints its figures (``encoder-parity:`` lines, collected by
tools/encoder_parity.py into profiles/encoder_parity.txt) before it asserts.  Bounds: see encoder_cases.py."""
import contextlib
import math
import os

import pytest
import torch

import encoder_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
SENTINEL = K.SENTINEL
NAME = K.NAME
PAD = 64                          # sentinel floats before and after a 1-D f32 output


def ops():
    from w2v2_speaker_amd import ops as o
    return o


def say(line: str) -> None:
    print("encoder-parity: " + line)


def host(t: torch.Tensor) -> torch.Tensor:
    torch.cuda.synchronize()
    return t.detach().float().cpu().to(F64)


class Worst:
    """The measurement closest to (or furthest past) its bound."""

    def __init__(self):
        self.ratio, self.err, self.bound, self.item = -1.0, 0.0, 0.0, ""

    def add(self, err, bound, item: str) -> None:
        """Scalars, or tensors of one shape (``bound`` may be a scalar): the element with the largest err / bound."""
        if isinstance(err, torch.Tensor):
            err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf)).flatten()
            if err.numel() == 0:
                return
            bound = bound.flatten() if isinstance(bound, torch.Tensor) else torch.full_like(err, float(bound))
            q = torch.where(err == 0, torch.zeros_like(err), err / bound)
            i = int(q.argmax())
            err, bound = float(err[i]), float(bound[i])
        if not math.isfinite(err):
            err = math.inf
        ratio = 0.0 if err == 0 else (err / bound if bound > 0 else math.inf)
        if ratio > self.ratio:
            self.ratio, self.err, self.bound, self.item = ratio, err, bound, item

    def __str__(self):
        return f"{self.err:.2e} bound {self.bound:.2e} ({self.item})"

    @property
    def ok(self) -> bool:
        return self.ratio <= 1.0


def guarded(rows: int, C: int, dtype):
    """-> (whole buffer [rows + 2, C], the [rows, C] view between one sentinel row before and one after), all sentinel."""
    buf = torch.full((rows + 2, C), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[1:rows + 1]


def guarded_1d(n: int):
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[PAD:PAD + n]


def guards_intact(*bufs) -> bool:
    torch.cuda.synchronize()
    ok = True
    for buf in bufs:
        if buf.dim() == 1:
            ok = ok and bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())
        else:
            ok = ok and bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())
    return ok


_MASKS = {}


def ln_device_mask(M: int, H: int) -> torch.Tensor:
    """[M, H] f32 of 0 or 1 / (1 - p): ops.dropout_ on ones draws the (seed, element index) stream of the LN kernels."""
    if (M, H) not in _MASKS:
        ones = torch.ones(M, H, device=DEV)
        ops().dropout_(ones, K.LN_P, K.LN_SEED)
        torch.cuda.synchronize()
        _MASKS[M, H] = ones.cpu()
    return _MASKS[M, H]


# ================================================================================================ 1. layer norm forward
def _ln_fwd(x, r, gamma, beta, dtype, p):
    """-> dict of the device results (float64 on the host) and whether every sentinel survived."""
    o = ops()
    M, H = x.shape
    rbuf, rv = guarded(M, H, dtype)
    if r is not None:
        rv.copy_(r.to(dtype))
    ybuf, y = guarded(M, H, dtype)
    mbuf, mean = guarded_1d(M)
    sbuf, rstd = guarded_1d(M)
    o.layernorm_fwd(x.to(dtype).to(DEV), None if r is None else rv, gamma.to(DEV), beta.to(DEV), y, mean, rstd, K.EPS, p,
                    K.LN_SEED)
    intact = guards_intact(rbuf, ybuf, mbuf, sbuf)
    return dict(r=rv, y=y, mean=mean, rstd=rstd, intact=intact)


@pytest.mark.parametrize("cls", K.LN_CLASSES)
@pytest.mark.parametrize("H", K.LN_H)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=NAME.get)
def test_layernorm_fwd_vs_float64(dtype, H, cls):
    """ops.layernorm_fwd without residual, with one, and with a dropped-out one, against the float64 LayerNorm of the
    UNROUNDED sum x + r * mask: the stored sum bit for bit, mean / rstd within 2^-22 + 8 x an f32 two-pass, y per row."""
    gamma, beta = K.ln_params(H)
    intact = True
    lines = []
    for variant in K.LN_FWD_VARIANTS:
        p = K.LN_P if variant.endswith("dropout") else 0.0
        runs, yard_m, yard_r = [], 0.0, 0.0
        for M in K.LN_M_SMALL:
            x, r = K.ln_fwd_inputs(cls, M, H, dtype, variant)
            mask = ln_device_mask(M, H) if p > 0 else None
            ref = K.ln_forward(x, r, mask, gamma, beta)
            e_m, e_r = K.ln_stats_errors(*K.ln_ideal_f32_stats(x if r is None else K.ln_f32_sums(x, r, mask)[0]), ref)
            yard_m, yard_r = max(yard_m, e_m), max(yard_r, e_r)
            runs.append((M, x, r, mask, ref, _ln_fwd(x, r, gamma, beta, dtype, p)))
        bm, br = K.STATS_FLOOR + K.STATS_ORDER * yard_m, K.STATS_FLOOR + K.STATS_ORDER * yard_r
        wm, wr, wy = Worst(), Worst(), Worst()
        stored_bad, const_bad, two_ways = [], [], 0
        for M, x, r, mask, ref, got in runs:
            intact = intact and got["intact"]
            e_m, e_r = K.ln_stats_errors(host(got["mean"]), host(got["rstd"]), ref)
            wm.add(e_m, bm, f"M={M}")
            wr.add(e_r, br, f"M={M}")
            y = host(got["y"])
            wy.add(K.sliced_rel_l2(y, ref.y, 1)[0], K.ln_y_bound(ref, dtype), f"M={M}")
            if r is not None:       # the stored sum: one of the two f32 evaluations, rounded once to the activation type
                a, b = (t.to(dtype).float() for t in K.ln_f32_sums(x, r, mask))
                s_dev = got["r"].float().cpu()
                two_ways += int((a != b).sum())
                if not bool(((s_dev == a) | (s_dev == b)).all()):
                    stored_bad.append(M)
            if cls == "const" and not (bool(torch.isfinite(y).all()) and torch.equal(y, beta.to(dtype).to(F64).expand(M, H))):
                const_bad.append(M)
        lines.append(f"{variant}: |d mean| * rstd {wm}; rel |d rstd| {wr}; y per row {wy}"
                     + ("" if r is None else f"; stored sum bit-equal {math.inf if stored_bad else 0} ({two_ways} elements "
                                             f"where fma and mul+add differ)"))
        say(f"layernorm fwd {NAME[dtype]} H={H} {cls} " + lines[-1])
        assert not stored_bad, f"stored sum is not x + r * mask rounded once: M in {stored_bad}"
        assert not const_bad, f"zero-variance rows: y is not beta: M in {const_bad}"
        assert wm.ok and wr.ok and wy.ok, lines[-1]
    assert intact, "a sentinel next to r, y, mean or rstd was written"


# ================================================================================================ 2. layer norm backward
def _ln_bwd(c, dtype, mode: str, p: float, with_dr: bool):
    """One backward launch (plus its fold) on sentinel-guarded ds / d_r / workspace and pre-filled dgamma / dbeta.
    immediate: the C entry with a workspace of this test's own; deferred: ops.layernorm_bwd through LnFoldGroup;
    none: dgamma / dbeta not requested."""
    o = ops()
    M, H = c.s.shape
    dy, s = c.dy.to(dtype).to(DEV), c.s.to(dtype).to(DEV)
    mean, rstd, gamma = c.mean.to(DEV), c.rstd.to(DEV), c.gamma.to(DEV)
    dsbuf, ds = guarded(M, H, dtype)
    drbuf, dr = guarded(M, H, dtype)
    dg, db = (t.clone().to(DEV) for t in K.ln_prefill(H))
    bufs, rows_written = [dsbuf, drbuf], None
    if mode == "immediate":
        nfl = o.lib().w2v2_layernorm_bwd_workspace_floats(H)
        wsbuf, ws = guarded(nfl // H, H, torch.float32)
        rc = o.lib().w2v2_layernorm_bwd(dy.data_ptr(), s.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                        ds.data_ptr(), dr.data_ptr() if with_dr else None, dg.data_ptr(), db.data_ptr(),
                                        ws.data_ptr(), M, H, p, K.LN_SEED, o.dt(dy), o.stream())
        assert rc == 0, o.lib().w2v2_last_error()
        torch.cuda.synchronize()
        rows_written = int((ws != SENTINEL).any(dim=1).sum())
        bufs.append(wsbuf)
    elif mode == "deferred":
        grp = o.LnFoldGroup(H, DEV)
        o.layernorm_bwd(dy, s, mean, rstd, gamma, ds, dr if with_dr else None, dg, db, p, K.LN_SEED, defer_to=grp)
        grp.fold()
    else:
        o.layernorm_bwd(dy, s, mean, rstd, gamma, ds, dr if with_dr else None, None, None, p, K.LN_SEED)
    intact = guards_intact(*bufs)
    return SimpleRun(ds=ds, dr=dr if with_dr else None, dg=dg, db=db, intact=intact, rows_written=rows_written)


class SimpleRun:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def same_bits(self, other, fields) -> bool:
        torch.cuda.synchronize()
        return all(torch.equal(getattr(self, f), getattr(other, f)) for f in fields if getattr(self, f) is not None)


def _judge_ln_bwd(c, run, mask, dtype, mode, w, item):
    """ds / d_r per row, dgamma / dbeta per column (prefill + reference, on sum |terms| with the prefill as one of them)."""
    ref = c.ref
    bound = K.ln_ds_bound(dtype)
    ds = host(run.ds)
    w["ds"].add(K.sliced_rel_l2(ds, ref.ds, 1)[0], bound, item)
    if run.dr is not None:
        dr = host(run.dr)
        w["d_r"].add(K.sliced_rel_l2(dr, ref.ds * mask.to(F64), 1)[0], bound, item)
        # the zero pattern of d_r is the mask's, element by element (wherever ds itself is not zero)
        wrong = ((dr != 0) != (mask != 0)) & (ds != 0)
        w["pattern"].add(float(wrong.sum()), 0.5, item)
    if mode != "none":
        pg, pb = (t.to(F64) for t in K.ln_prefill(c.s.shape[1]))
        w["dgamma"].add(K.sum_scale_error(host(run.dg), pg + ref.dgamma, pg.abs() + ref.terms_g), K.BWD_TOL, item)
        w["dbeta"].add(K.sum_scale_error(host(run.db), pb + ref.dbeta, pb.abs() + ref.terms_b), K.BWD_TOL, item)


@pytest.mark.parametrize("H", K.LN_H)
@pytest.mark.parametrize("dtype", K.DTYPES, ids=NAME.get)
def test_layernorm_bwd_vs_float64(dtype, H):
    """w2v2_layernorm_bwd on the s, mean and rstd it is handed, every input class at M = 1, 3, 37 and the two that tell rows
    apart at M = 2 * 4 * cap + 5.  The immediate fold with dropout is compared with float64 in full; the deferred fold, the
    launch without dgamma and the one without d_r must give the same bits wherever they compute the same thing (and the
    launch without dgamma is compared in full where it is another kernel); every launch runs twice."""
    o = ops()
    nfl = o.lib().w2v2_layernorm_bwd_workspace_floats(H)
    assert nfl == max(K.LN_BWD_BLOCKS, K.LN_BWD_BLOCKS_Q) * 2 * H          # the caps the large M is derived from
    big = K.ln_large_m(H)
    assert big == 2 * 4 * K.ln_block_cap(H) + 5
    w = {k: Worst() for k in ("ds", "d_r", "pattern", "dgamma", "dbeta")}
    intact, repeat_bad, twin_bad, rows_bad = True, [], [], []
    for M in K.ln_bwd_ms(H):
        for cls in (K.LN_CLASSES if M != big else K.LN_LARGE_CLASSES):
            c = K.ln_bwd_case(cls, M, H, dtype)
            mask = ln_device_mask(M, H)
            item = f"{cls} M={M}"
            runs = {}
            for mode, p, with_dr in (("immediate", K.LN_P, True), ("deferred", K.LN_P, True), ("none", K.LN_P, True),
                                     ("immediate", 0.0, False)):
                a, b = _ln_bwd(c, dtype, mode, p, with_dr), _ln_bwd(c, dtype, mode, p, with_dr)
                intact = intact and a.intact and b.intact
                if not a.same_bits(b, ("ds", "dr", "dg", "db")):
                    repeat_bad.append((item, mode, p))
                runs[mode, with_dr] = a
            first = runs["immediate", True]
            _judge_ln_bwd(c, first, mask, dtype, "immediate", w, item)
            # the partial rows the launch wrote: two per workgroup, min(ceil(M / 4), cap) workgroups
            if first.rows_written != 2 * min(-(-M // 4), K.ln_block_cap(H)):
                rows_bad.append((item, first.rows_written))
            if not first.same_bits(runs["deferred", True], ("ds", "dr", "dg", "db")):
                twin_bad.append((item, "deferred fold"))
            if not first.same_bits(runs["immediate", False], ("ds", "dg", "db")):
                twin_bad.append((item, "no d_r, p = 0"))
            none = runs["none", True]
            if K.ln_bwd_kernel(dtype, H, "none") == K.ln_bwd_kernel(dtype, H, "immediate"):
                if not first.same_bits(none, ("ds", "dr")):
                    twin_bad.append((item, "dgamma not requested"))
            else:                                   # 16-bit at a quad width: another kernel, judged on its own
                _judge_ln_bwd(c, none, mask, dtype, "none", w, item + " (no dgamma)")
            if not torch.equal(none.dg.cpu(), K.ln_prefill(H)[0]) or not torch.equal(none.db.cpu(), K.ln_prefill(H)[1]):
                twin_bad.append((item, "dgamma touched though not requested"))
    say(f"layernorm bwd {NAME[dtype]} H={H} ({K.ln_bwd_kernel(dtype, H, 'immediate')}"
        + (f", without dgamma {K.ln_bwd_kernel(dtype, H, 'none')}" if K.ln_bwd_kernel(dtype, H, 'none') != K.ln_bwd_kernel(dtype, H, 'immediate') else "")
        + f"), M up to {big}: ds per row {w['ds']}; d_r per row {w['d_r']}; d_r zeros not the mask's {w['pattern'].err:.0f} elements; "
        f"dgamma /sum|terms| {w['dgamma']}; dbeta /sum|terms| {w['dbeta']}; second run / deferred fold / other arguments "
        f"(bit-equal) {math.inf if repeat_bad or twin_bad else 0}")
    assert intact, "a sentinel row next to ds, d_r or the workspace was written"
    assert not rows_bad, f"partial rows written: {rows_bad}"
    assert not repeat_bad, f"a second run differs from the first: {repeat_bad}"
    assert not twin_bad, f"results that must be bit-equal differ: {twin_bad}"
    assert all(x.ok for x in w.values())


@pytest.mark.parametrize("entries", (1, 3))
@pytest.mark.parametrize("dtype,H,M", ((torch.float16, 768, 132), (torch.float32, 40, 5)), ids=("f16-768x132", "f32-40x5"))
def test_layernorm_bwd_fold_routes_give_the_same_bits(dtype, H, M, entries):
    """dgamma / dbeta of an immediate layernorm_bwd and of a deferred one folded through LnFoldGroup -- alone, or as one of
    three entries of one fold launch -- are bitwise equal: one fold kernel serves both routes, with the same lane walk over
    the partial rows (M = 132: 33 of them, one block lane takes two) and the same lane-order LDS fold."""
    o = ops()
    cases = [K.ln_bwd_case(cls, M, H, dtype) for cls in K.LN_CLASSES[:entries]]
    grp = o.LnFoldGroup(H, DEV)
    deferred = []
    for c in cases:
        dg, db = (t.clone().to(DEV) for t in K.ln_prefill(H))
        ds = torch.empty(M, H, dtype=dtype, device=DEV)
        o.layernorm_bwd(c.dy.to(dtype).to(DEV), c.s.to(dtype).to(DEV), c.mean.to(DEV), c.rstd.to(DEV), c.gamma.to(DEV), ds,
                        None, dg, db, 0.0, K.LN_SEED, defer_to=grp)
        deferred.append(SimpleRun(ds=ds, dg=dg, db=db))
    grp.fold()
    differ = []
    for cls, c, d in zip(K.LN_CLASSES, cases, deferred):
        first = _ln_bwd(c, dtype, "immediate", 0.0, False)
        assert first.intact
        if not first.same_bits(d, ("ds", "dg", "db")):
            differ.append(cls)
    say(f"layernorm bwd fold routes {NAME[dtype]} H={H} M={M}, {entries} deferred: entries that differ from the immediate "
        f"fold {differ}")
    assert not differ


@pytest.mark.parametrize("cls", K.LN_CHAIN_CLASSES)
@pytest.mark.parametrize("dtype", K.LP, ids=NAME.get)
def test_layernorm_chained_fwd_bwd(dtype, cls):
    """As training runs it: the forward (residual, dropout) takes its statistics from the unrounded sum and stores the sum
    rounded; the backward rebuilds x-hat from the stored sum with those statistics.  norm.hip states the cost: x-hat is off
    by at most u(dtype) * |s| * rstd per element (on top of what the statistics' own bound allows); then the device backward
    on the device forward's outputs against float64 on the same."""
    wx, w = Worst(), {k: Worst() for k in ("ds", "d_r", "pattern", "dgamma", "dbeta")}
    intact = True
    for H in (64, 768, 1024):
        M = 37
        gamma, beta = K.ln_params(H)
        x, r = K.ln_fwd_inputs(cls, M, H, dtype, "residual+dropout")
        mask = ln_device_mask(M, H)
        ref = K.ln_forward(x, r, mask, gamma, beta)
        got = _ln_fwd(x, r, gamma, beta, dtype, K.LN_P)
        e_m, e_r = K.ln_stats_errors(*K.ln_ideal_f32_stats(K.ln_f32_sums(x, r, mask)[0]), ref)
        bm, br = K.STATS_FLOOR + K.STATS_ORDER * e_m, K.STATS_FLOOR + K.STATS_ORDER * e_r
        s_dev, mean_dev, rstd_dev = host(got["r"]), host(got["mean"]), host(got["rstd"])
        xh_true = (ref.s - ref.mean[:, None]) * ref.rstd[:, None]
        xh_dev = (s_dev - mean_dev[:, None]) * rstd_dev[:, None]
        bound = K.U[dtype] * ref.s.abs() * ref.rstd[:, None] + bm + br * xh_true.abs()
        wx.add((xh_dev - xh_true).abs(), bound, f"H={H}")
        c = K.SimpleNamespace(s=s_dev, dy=K.rnd(M, H, seed=5).to(dtype).to(F64), gamma=gamma, mean=got["mean"].cpu(),
                              rstd=got["rstd"].cpu())
        c.ref = K.ln_backward(c.dy, s_dev, mean_dev, rstd_dev, gamma.to(F64))
        run = _ln_bwd(c, dtype, "immediate", K.LN_P, True)
        intact = intact and got["intact"] and run.intact
        _judge_ln_bwd(c, run, mask, dtype, "immediate", w, f"H={H}")
    say(f"layernorm chained fwd -> bwd {NAME[dtype]} {cls}: |x-hat from the stored sum - x-hat| per element {wx}; "
        f"ds per row {w['ds']}; d_r per row {w['d_r']}; dgamma /sum|terms| {w['dgamma']}; dbeta /sum|terms| {w['dbeta']}")
    assert intact
    assert wx.ok and all(x.ok for x in w.values())


def test_layernorm_rejected_arguments_return_an_error_before_any_launch():
    o = ops()
    t = torch.zeros(4, 1040, device=DEV)
    v = torch.zeros(1040, device=DEV)
    for H in (12, 1032):
        rc = o.lib().w2v2_layernorm_fwd(t.data_ptr(), None, v.data_ptr(), v.data_ptr(), t.data_ptr(), v.data_ptr(), v.data_ptr(),
                                        2, H, K.EPS, 0.0, 0, o.dt(t), o.stream())
        assert rc != 0 and b"unsupported" in o.lib().w2v2_last_error()
        rc = o.lib().w2v2_layernorm_bwd(t.data_ptr(), t.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), t.data_ptr(), None,
                                        None, None, None, 2, H, 0.0, 0, o.dt(t), o.stream())
        assert rc != 0 and b"unsupported" in o.lib().w2v2_last_error()
    rc = o.lib().w2v2_layernorm_fwd(t.data_ptr(), None, v.data_ptr(), v.data_ptr(), t.data_ptr(), v.data_ptr(), v.data_ptr(),
                                    2, 1024, K.EPS, 1.0, 0, o.dt(t), o.stream())
    assert rc != 0 and b"dropout" in o.lib().w2v2_last_error()
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


# ================================================================================================ 3. attention
@contextlib.contextmanager
def attn_env(geom=None, no_dma=False):
    """W2V2_ATTN_GEOM / W2V2_ATTN_KV_NO_DMA are read on every call; whatever they were comes back afterwards."""
    names = ("W2V2_ATTN_GEOM", "W2V2_ATTN_KV_NO_DMA")
    old = {k: os.environ.get(k) for k in names}
    try:
        for k in names:
            os.environ.pop(k, None)
        if geom is not None:
            os.environ["W2V2_ATTN_GEOM"] = geom
        if no_dma:
            os.environ["W2V2_ATTN_KV_NO_DMA"] = "1"
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


FWD_CONFIGS = (("32", False), ("64", False), (None, False))
BWD_CONFIGS = (("32", False), ("32", True), ("64", False), (None, False))      # (geometry, LDS-DMA off)


def config_name(geom, no_dma) -> str:
    return ("unforced" if geom is None else f"geom {geom}") + (" no DMA" if no_dma else "")


def _attn_fwd(qkv: torch.Tensor, T: int, dtype, p: float = 0.0):
    """-> (ctx [B, T, H] and lse [B * heads * T] device views, sentinels intact)."""
    cbuf, cv = guarded(K.AT_B * T, K.AT_H, dtype)
    lbuf, lse = guarded_1d(K.AT_B * K.AT_HEADS * T)
    ctx = cv.view(K.AT_B, T, K.AT_H)
    ops().attention_fwd(qkv, ctx, lse, K.AT_B, T, K.AT_HEADS, K.AT_D, K.AT_SCALE, p, K.AT_SEED)
    return ctx, lse, guards_intact(cbuf, lbuf)


def _attn_bwd(qkv, ctx, dctx, lse, T: int, dtype, p: float = 0.0):
    """-> (dqkv [B, T, 3 H] and delta [B * heads * T] device views, sentinels intact)."""
    gbuf, gv = guarded(K.AT_B * T, 3 * K.AT_H, dtype)
    dbuf, delta = guarded_1d(K.AT_B * K.AT_HEADS * T)
    dqkv = gv.view(K.AT_B, T, 3 * K.AT_H)
    ops().attention_bwd(qkv, ctx, dctx, lse, dqkv, delta, K.AT_B, T, K.AT_HEADS, K.AT_D, K.AT_SCALE, p, K.AT_SEED)
    return dqkv, delta, guards_intact(gbuf, dbuf)


def split3(dqkv: torch.Tensor):
    g = host(dqkv)
    return [K.heads(g[..., i * K.AT_H:(i + 1) * K.AT_H]) for i in range(3)]


class Ratio:
    """Worst kernel error over the ideal 16-bit attention's error on the same row (both over the f32 term as well, so that
    the bound YARD_FACTOR x yardstick + F32_TOL is met exactly when this is at most YARD_FACTOR)."""

    def __init__(self):
        self.v = 0.0

    def add(self, err, yerr, f32_term):
        q = err / (yerr + f32_term / K.YARD_FACTOR)
        self.v = max(self.v, float(torch.where(torch.isfinite(q), q, torch.full_like(q, math.inf)).max()))


def judge_rows(w: Worst, rat: Ratio, got, ref, yard, name, c, item):
    err, yerr = K.slice_errors(got, ref, name, c)[0], K.yard_errors(yard, ref, name, c)
    w.add(err, K.yard_bound(yard, ref, name, c), item)
    rat.add(err, yerr, K.f32_term(ref, name, c))


def judge_forward(c, ctx, lse, T, w, rat, item):
    judge_rows(w["ctx"], rat["ctx"], K.heads(host(ctx)), c.ctx, c.y_ctx, "ctx", c, item)
    got = host(lse).view(K.AT_B, K.AT_HEADS, T)
    w["lse"].add((got - c.lse).abs(), K.lse_bound(c.lse, c.e_lse), item)


def judge_backward(c, dqkv, delta, T, w, rat, item):
    for name, got, ref, yard in zip(("dq", "dk", "dv"), split3(dqkv), (c.dq, c.dk, c.dv), (c.y_dq, c.y_dk, c.y_dv)):
        judge_rows(w[name], rat[name], got, ref, yard, name, c, item)
    got = host(delta).view(K.AT_B, K.AT_HEADS, T)
    w["delta"].add(K.sum_scale_error(got, c.delta, c.delta_terms), K.F32_TOL, item)


def summary(w, rat) -> str:
    return "; ".join(f"{k} {v}" + (f" kernel/yardstick {rat[k].v:.2f}" if k in rat else "") for k, v in w.items())


@pytest.mark.parametrize("cls", K.AT_CLASSES)
@pytest.mark.parametrize("dtype", K.LP, ids=NAME.get)
def test_attention_fwd_vs_float64(dtype, cls):
    """ops.attention_fwd at every T of the case list under both geometries and unforced: every ctx row within 2 x the ideal
    16-bit attention's error on that row, every lse within 2^-22 max(1, |lse|) + 8 x an f32 evaluation's error; the unforced
    launch gives the bits of the geometry the selection rule names."""
    w = {k: Worst() for k in ("ctx", "lse")}
    rat = {"ctx": Ratio()}
    intact, rule_bad, differ = True, [], 0
    for T in K.AT_T:
        c = K.attn_case(cls, T, dtype)
        qkv = c.qkv.to(dtype).to(DEV)
        out = {}
        for geom, no_dma in FWD_CONFIGS:
            with attn_env(geom, no_dma):
                ctx, lse, ok = _attn_fwd(qkv, T, dtype)
            intact = intact and ok
            judge_forward(c, ctx, lse, T, w, rat, f"T={T} {config_name(geom, no_dma)}")
            out[geom] = (ctx, lse)
        want = "32" if K.small_geom(T) else "64"
        if not all(torch.equal(a, b) for a, b in zip(out[None], out[want])):
            rule_bad.append(T)
        differ += int(not all(torch.equal(a, b) for a, b in zip(out["32"], out["64"])))
    say(f"attention fwd {NAME[dtype]} {cls}: {summary(w, rat)}; unforced = the selected geometry (bit-equal) "
        f"{math.inf if rule_bad else 0} (the two geometries differ in some bit at {differ} of {len(K.AT_T)} lengths)")
    assert intact, "a sentinel next to ctx or lse was written"
    assert not rule_bad, f"the unforced launch is not the geometry attn_small_geom names at T in {rule_bad}"
    assert all(x.ok for x in w.values())


@pytest.mark.parametrize("cls", K.AT_CLASSES)
@pytest.mark.parametrize("dtype", K.LP, ids=NAME.get)
def test_attention_bwd_vs_float64(dtype, cls):
    """ops.attention_bwd on a ctx (rounded to the type) and an lse (rounded to f32) computed by the float64 reference, under
    both geometries, with and without LDS-DMA tile loads, and unforced: every dQ / dK / dV row within 2 x the ideal 16-bit
    backward's error on that row, delta within 2e-6 of sum |dO ctx|; a second run repeats the first bit for bit."""
    w = {k: Worst() for k in ("dq", "dk", "dv", "delta")}
    rat = {k: Ratio() for k in ("dq", "dk", "dv")}
    intact, repeat_bad, rule_bad, dma_bad = True, [], [], []
    for T in K.AT_T:
        c = K.attn_case(cls, T, dtype)
        qkv, dctx = c.qkv.to(dtype).to(DEV), c.dctx.to(dtype).to(DEV)
        ctx = K.unheads(c.ctx16).to(dtype).to(DEV).contiguous()
        lse = c.lse32.float().to(DEV).reshape(-1).contiguous()
        out = {}
        for geom, no_dma in BWD_CONFIGS:
            with attn_env(geom, no_dma):
                dqkv, delta, ok = _attn_bwd(qkv, ctx, dctx, lse, T, dtype)
                dqkv2, delta2, ok2 = _attn_bwd(qkv, ctx, dctx, lse, T, dtype)
            intact = intact and ok and ok2
            if not (torch.equal(dqkv, dqkv2) and torch.equal(delta, delta2)):
                repeat_bad.append((T, config_name(geom, no_dma)))
            judge_backward(c, dqkv, delta, T, w, rat, f"T={T} {config_name(geom, no_dma)}")
            out[geom, no_dma] = (dqkv, delta)
        want = "32" if K.small_geom(T) else "64"
        if not all(torch.equal(a, b) for a, b in zip(out[None, False], out[want, False])):
            rule_bad.append(T)
        if not all(torch.equal(a, b) for a, b in zip(out["32", False], out["32", True])):
            dma_bad.append(T)
    say(f"attention bwd {NAME[dtype]} {cls}: {summary(w, rat)}; second run / unforced = selected geometry / DMA = register "
        f"staging (bit-equal) {math.inf if repeat_bad or rule_bad or dma_bad else 0}")
    assert intact, "a sentinel next to dqkv or delta was written"
    assert not repeat_bad, f"a second run differs from the first: {repeat_bad}"
    assert not rule_bad, f"the unforced launch is not the geometry attn_small_geom names at T in {rule_bad}"
    assert not dma_bad, f"LDS-DMA tile loads change the result at T in {dma_bad}"
    assert all(x.ok for x in w.values())


@pytest.mark.parametrize("cls", K.AT_CHAIN_CLASSES)
@pytest.mark.parametrize("dtype", K.LP, ids=NAME.get)
def test_attention_chained_fwd_bwd(dtype, cls):
    """As training runs it (nothing forced): the device forward's ctx and lse go into the device backward; the result is
    held to the float64 backward of exactly those inputs, so the two kernels must agree on the layout and the meaning of
    what passes between them (lse in natural log per (b, head, q), ctx per (b, q, head))."""
    w = {k: Worst() for k in ("ctx", "lse", "dq", "dk", "dv", "delta")}
    rat = {k: Ratio() for k in ("ctx", "dq", "dk", "dv")}
    intact = True
    for T in K.AT_CHAIN_T:
        c = K.attn_case(cls, T, dtype)
        qkv, dctx = c.qkv.to(dtype).to(DEV), c.dctx.to(dtype).to(DEV)
        ctx, lse, ok = _attn_fwd(qkv, T, dtype)
        judge_forward(c, ctx, lse, T, w, rat, f"T={T}")
        dqkv, delta, ok2 = _attn_bwd(qkv, ctx, dctx, lse, T, dtype)
        intact = intact and ok and ok2
        c2 = K.attn_backward_of(c, K.heads(host(ctx)), host(lse).view(K.AT_B, K.AT_HEADS, T))
        judge_backward(c2, dqkv, delta, T, w, rat, f"T={T}")
    say(f"attention chained fwd -> bwd {NAME[dtype]} {cls}: {summary(w, rat)}")
    assert intact
    assert all(x.ok for x in w.values())


# ------------------------------------------------------------------------------------------------ dropout
def _probe_fwd(T: int, dtype) -> torch.Tensor:
    """The forward's keep mask [B, h, q, key]: q = k = 0 makes P uniform, one-hot value rows make ctx a window of Pdrop."""
    m = torch.zeros(K.AT_B, K.AT_HEADS, T, T, dtype=F64)
    for k0 in range(0, T, K.AT_D):
        n = min(K.AT_D, T - k0)
        probe = torch.zeros(K.AT_B, T, 3 * K.AT_H)
        for h in range(K.AT_HEADS):
            probe[:, k0:k0 + n, 2 * K.AT_H + h * K.AT_D:2 * K.AT_H + h * K.AT_D + n] = torch.eye(n)
        ctx, _, _ = _attn_fwd(probe.to(dtype).to(DEV), T, dtype, K.AT_P)
        m[..., k0:k0 + n] = (K.heads(host(ctx))[..., :n] > 0).double()
    return m


def _probe_bwd(T: int, dtype):
    """The keep masks of the two backward kernels, read directly.  dK/dV kernel: with q = k = v = 0, ctx = 0 and
    lse = log T, one-hot dO rows make dV[key, c] = Pdrop[q0 + c, key].  dQ kernel: with V = ones, dO = 1 / 64 (dP = 1),
    ctx = 0 (delta = 0) and one-hot key rows, dQ[q, c] = scale / T * keep-scale[q, k0 + c]."""
    B, Hh, H, d = K.AT_B, K.AT_HEADS, K.AT_H, K.AT_D
    mkv, mdq = torch.zeros(B, Hh, T, T, dtype=F64), torch.zeros(B, Hh, T, T, dtype=F64)
    ctx0 = torch.zeros(B, T, H, dtype=dtype, device=DEV)
    lse = torch.full((B * Hh * T,), math.log(T), device=DEV)
    zeros = torch.zeros(B, T, 3 * H, dtype=dtype, device=DEV)
    for r0 in range(0, T, d):
        n = min(d, T - r0)
        dctx = torch.zeros(B, T, H)
        qkv = torch.zeros(B, T, 3 * H)
        qkv[..., 2 * H:] = 1.0
        for h in range(Hh):
            dctx[:, r0:r0 + n, h * d:h * d + n] = torch.eye(n)
            qkv[:, r0:r0 + n, H + h * d:H + h * d + n] = torch.eye(n)
        dqkv, _, _ = _attn_bwd(zeros, ctx0, dctx.to(dtype).to(DEV), lse, T, dtype, K.AT_P)
        dv = split3(dqkv)[2]                                              # [B, h, key, c] = Pdrop[r0 + c, key]
        mkv[:, :, r0:r0 + n, :] = (dv[..., :n] > 0).double().transpose(2, 3)
        ones = torch.full((B, T, H), 1.0 / d).to(dtype).to(DEV)
        dqkv, _, _ = _attn_bwd(qkv.to(dtype).to(DEV), ctx0, ones, lse, T, dtype, K.AT_P)
        mdq[..., r0:r0 + n] = (split3(dqkv)[0][..., :n] > 0).double()
    return mkv, mdq


@pytest.mark.parametrize("T", K.AT_DROP_T)
@pytest.mark.parametrize("dtype", K.LP, ids=NAME.get)
def test_attention_dropout_mask_and_values(dtype, T):
    """p = 0.1: the keep mask read back from the forward (one-hot V), from the dK/dV kernel (one-hot dO) and from the dQ
    kernel (one-hot K) is ONE mask, under both geometries and with or without LDS-DMA; with that mask in the float64
    reference and in the yardstick, forward and backward are held to the same per-row bounds as without dropout."""
    masks = {}
    for geom, no_dma in BWD_CONFIGS[:3]:
        with attn_env(geom, no_dma):
            mkv, mdq = _probe_bwd(T, dtype)
            masks[config_name(geom, no_dma)] = (_probe_fwd(T, dtype), mkv, mdq)
    mask = masks["geom 32"][0]
    keep_rate = float(mask.mean())
    differ = [(name, which) for name, ms in masks.items() for which, m in zip(("fwd", "dK/dV", "dQ"), ms) if not torch.equal(m, mask)]
    c = K.attn_case_of("gauss", T, dtype, mask, 1 - K.AT_P)
    qkv, dctx = c.qkv.to(dtype).to(DEV), c.dctx.to(dtype).to(DEV)
    ctx16 = K.unheads(c.ctx16).to(dtype).to(DEV).contiguous()
    lse32 = c.lse32.float().to(DEV).reshape(-1).contiguous()
    w = {k: Worst() for k in ("ctx", "lse", "dq", "dk", "dv", "delta")}
    rat = {k: Ratio() for k in ("ctx", "dq", "dk", "dv")}
    intact, repeat_bad = True, []
    for geom, no_dma in BWD_CONFIGS:
        item = config_name(geom, no_dma)
        with attn_env(geom, no_dma):
            ctx, lse, ok = _attn_fwd(qkv, T, dtype, K.AT_P)
            dqkv, delta, ok2 = _attn_bwd(qkv, ctx16, dctx, lse32, T, dtype, K.AT_P)
            dqkv2, delta2, ok3 = _attn_bwd(qkv, ctx16, dctx, lse32, T, dtype, K.AT_P)
        intact = intact and ok and ok2 and ok3
        if not (torch.equal(dqkv, dqkv2) and torch.equal(delta, delta2)):
            repeat_bad.append(item)
        judge_forward(c, ctx, lse, T, w, rat, item)
        judge_backward(c, dqkv, delta, T, w, rat, item)
    tol = 4 * math.sqrt(K.AT_P * (1 - K.AT_P) / mask.numel()) + 0.5 / 65536      # four sigma, and the 16-bit threshold
    say(f"attention dropout {NAME[dtype]} T={T}: keep rate {keep_rate:.4f} (want {1 - K.AT_P} +- {tol:.4f}); masks of fwd / dK,dV / dQ "
        f"under {', '.join(masks)} (bit-equal) {math.inf if differ else 0}; {summary(w, rat)}")
    assert not differ, f"masks that differ from the forward's under geometry 32: {differ}"
    assert abs(keep_rate - (1 - K.AT_P)) < tol
    assert intact and not repeat_bad, repeat_bad
    assert all(x.ok for x in w.values())


def test_attention_rejected_arguments_return_an_error_before_any_launch():
    o = ops()
    B, T, Hh = 1, 8, 2
    qkv = torch.zeros(B, T, 3 * Hh * 64, dtype=torch.bfloat16, device=DEV)
    ctx = torch.full((B, T, Hh * 64), SENTINEL, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B * Hh * T,), SENTINEL, device=DEV)
    lib = o.lib()
    for d, p, dt, word in ((32, 0.0, o.dt(qkv), b"head dim 64"), (64, 1.0, o.dt(qkv), b"dropout"),
                           (64, 0.0, o.dt(lse), b"16-bit")):
        rc = lib.w2v2_attention_fwd(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), B, T, Hh, d, 0.125, p, 0, dt, o.stream())
        assert rc != 0 and word in lib.w2v2_last_error(), lib.w2v2_last_error()
        rc = lib.w2v2_attention_bwd(qkv.data_ptr(), ctx.data_ptr(), ctx.data_ptr(), lse.data_ptr(), qkv.data_ptr(), lse.data_ptr(),
                                    B, T, Hh, d, 0.125, p, 0, dt, o.stream())
        assert rc != 0 and word in lib.w2v2_last_error(), lib.w2v2_last_error()
    torch.cuda.synchronize()
    assert bool((ctx == SENTINEL).all()) and bool((lse == SENTINEL).all()) and float(qkv.float().abs().max()) == 0.0
