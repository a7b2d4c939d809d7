"""GPU unit tests of the optimiser options (csrc/optim.hip): the two-launch global gradient norm, the general optimiser
step (Adam with L2 weight decay, SGD, the clip coefficient folded in) and SGD under the loss-scale record.  The truth is
torch itself on the CPU: torch.linalg.vector_norm in float64, torch.optim.Adam / torch.optim.SGD and
torch.nn.utils.clip_grad_norm_.  Shapes are the smallest at which the kernels can go wrong: a tail only, vectors + tail
in one workgroup, many workgroups + tail.  Run with -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 4 * 1000 + 3


def ops():
    from w2v2_speaker_amd import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _norm(o, g, scaler, max_norm, grad_scale=0.5):
    n = g.numel()
    state = torch.full((2,), -1.0, device=DEV)
    partials = torch.zeros(o.grad_norm_partials(n), dtype=torch.float64, device=DEV)
    o.grad_norm(g, n, state, partials, grad_scale, scaler, max_norm)
    torch.cuda.synchronize()
    return state


# ------------------------------------------------------------------------------------------------- global norm
@pytest.mark.parametrize("n", [3, 4 * 1000 + 3, 2 ** 20 + 1])
def test_grad_norm_matches_float64_and_is_reproducible(n):
    """norm_state[0] within 1e-6 relative of the float64 norm of the unscaled gradient (double accumulation leaves the
    f32 rounding of the stored result, 6e-8, and of the per-element pre-scaling -- exact here, the factor 0.5 / 256 is a
    power of two), the coefficient = min(1, c / (norm + 1e-6)) to the same tolerance and exactly 1 when it does not
    clip; two launches give the same bits.  2^20 + 1 elements: 256 workgroups, i.e. more partials than one wavefront."""
    o = ops()
    assert o.grad_norm_partials(n) == {3: 1, 4003: 1, 2 ** 20 + 1: 256}[n]
    g_host = rnd(n, seed=n % 97)
    g = g_host.to(DEV)
    scaler = torch.tensor([256.0, 0, 0, 0, 0, 0, 0, 0], device=DEV)
    want = float(torch.linalg.vector_norm(g_host.double() * (0.5 / 256.0)))
    clip = 0.25 * want
    s_clip = _norm(o, g, scaler, clip)
    s_free = _norm(o, g, scaler, 4.0 * want)
    s_only = _norm(o, g, scaler, 0.0)                   # max_norm <= 0: norm only
    again = _norm(o, g, scaler, clip)
    print(f"n={n}: norm {float(s_clip[0]):.9e} vs float64 {want:.9e}  rel {abs(float(s_clip[0]) - want) / want:.2e}")
    assert abs(float(s_clip[0]) - want) <= 1e-6 * want
    want_coef = min(1.0, clip / (want + 1e-6))
    assert abs(float(s_clip[1]) - want_coef) <= 1e-6 * want_coef
    assert float(s_free[1]) == 1.0 and float(s_only[1]) == 1.0
    assert torch.equal(s_free[0], s_clip[0]) and torch.equal(s_only[0], s_clip[0])
    assert torch.equal(again, s_clip)
    assert scaler.tolist() == [256.0, 0, 0, 0, 0, 0, 0, 0]          # a finite norm leaves the record alone
    # without a record the factor is plain grad_scale
    s_plain = _norm(o, g, None, 0.0, grad_scale=0.5)
    assert abs(float(s_plain[0]) - 256.0 * want) <= 1e-6 * 256.0 * want


@pytest.mark.parametrize("n", [3, 4 * 1000 + 3, 2 ** 20 + 1])
@pytest.mark.parametrize("where", ["last", "first"])
def test_grad_norm_non_finite_sets_found_inf_and_zero_coefficient(n, where):
    """One inf at the very last index (in the scalar tail) or at index 0: found_inf = 1 and a zero coefficient."""
    o = ops()
    g = rnd(n, seed=5).to(DEV)
    g[n - 1 if where == "last" else 0] = float("inf")
    scaler = torch.tensor([256.0, 0, 0, 0, 0, 0, 0, 0], device=DEV)
    state = _norm(o, g, scaler, 1.0)
    assert float(scaler[1]) == 1.0 and float(state[1]) == 0.0 and not np.isfinite(float(state[0]))
    state = _norm(o, g, None, 0.0)                      # no record, norm only: the coefficient alone guards the step
    assert float(state[1]) == 0.0


# ------------------------------------------------------------------------------------------------- default path
@pytest.mark.parametrize("lp", [None, torch.bfloat16, torch.float16])
def test_optim_step_default_adam_is_adam_step_bit_for_bit(lp):
    o = ops()
    outs = []
    for general in (False, True):
        p = rnd(N, seed=1).to(DEV)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        pb = torch.zeros(N, dtype=lp, device=DEV) if lp is not None else None
        for i in range(3):
            gr = rnd(N, seed=10 + i).to(DEV)
            if general:
                o.optim_step("adam", p, gr, m, v, pb, N, 1e-3, 0.9, 0.999, 1e-8, i + 1, grad_scale=0.5)
            else:
                o.adam_step(p, gr, m, v, pb, N, 1e-3, 0.9, 0.999, 1e-8, i + 1, grad_scale=0.5)
        torch.cuda.synchronize()
        outs.append((p, m, v) + ((pb,) if pb is not None else ()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ------------------------------------------------------------------------------------------------- against torch
VARIANTS = {
    "adam": dict(algo="adam"),
    "sgd_nesterov": dict(algo="sgd", momentum=0.9, nesterov=True),
    "sgd_dampening": dict(algo="sgd", momentum=0.9, dampening=0.1),
    "sgd_plain": dict(algo="sgd", momentum=0.0),
}


def _torch_run(variant, wd, max_norm, steps=3, lr=1e-3):
    ref = torch.nn.Parameter(rnd(N, seed=1))
    kw = dict(VARIANTS[variant])
    algo = kw.pop("algo")
    opt = (torch.optim.Adam([ref], lr=lr, weight_decay=wd) if algo == "adam"
           else torch.optim.SGD([ref], lr=lr, weight_decay=wd, **kw))
    for i in range(steps):
        ref.grad = rnd(N, seed=10 + i)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
    return ref.detach()


def _hip_run(o, variant, wd, max_norm, lp, steps=3, lr=1e-3):
    kw = dict(VARIANTS[variant])
    algo = kw.pop("algo")
    p = rnd(N, seed=1).to(DEV)
    m = torch.zeros_like(p) if (algo == "adam" or kw["momentum"] != 0) else None
    v = torch.zeros_like(p) if algo == "adam" else None
    pb = torch.zeros(N, dtype=lp, device=DEV)
    state = torch.zeros(2, device=DEV)
    partials = torch.zeros(o.grad_norm_partials(N), dtype=torch.float64, device=DEV)
    for i in range(steps):
        gr = rnd(N, seed=10 + i).to(DEV)
        if max_norm is not None:
            o.grad_norm(gr, N, state, partials, 1.0, None, max_norm)
        o.optim_step(algo, p, gr, m, v, pb, N, lr, kw.get("momentum", 0.9) if algo == "sgd" else 0.9, 0.999, 1e-8, i + 1,
                     weight_decay=wd, norm_state=state if max_norm is not None else None, **kw)
    torch.cuda.synchronize()
    return p, m, pb, state


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("max_norm", [None, 1.0, 1e3])
def test_optim_step_matches_torch(variant, wd, max_norm):
    """Three steps at lr 1e-3 over 4003 elements against torch.optim.Adam / SGD (+ clip_grad_norm_): atol 1e-6, the
    bound of the fused-Adam test at this size, step count and learning rate.  rnd gradients have norm ~63, so
    max_norm = 1 clips and 1e3 does not; the run that is below the threshold is bit-equal to a run without a norm
    record, and the 16-bit copy is the rounded master."""
    o = ops()
    lp = torch.float16 if wd else torch.bfloat16
    want = _torch_run(variant, wd, max_norm)
    p, m, pb, state = _hip_run(o, variant, wd, max_norm, lp)
    err = float((p.cpu() - want).abs().max())
    print(f"{variant} wd={wd} max_norm={max_norm}: max |p - torch| = {err:.2e}  norm {float(state[0]):.3f} coef {float(state[1]):.4f}")
    assert np.allclose(p.cpu().numpy(), want.numpy(), atol=1e-6, rtol=0)
    assert torch.equal(pb, p.to(lp))
    if max_norm == 1.0:
        assert 0.0 < float(state[1]) < 0.02
    if max_norm == 1e3:
        assert float(state[1]) == 1.0
        p2, m2, pb2, _ = _hip_run(o, variant, wd, None, lp)
        assert torch.equal(p, p2) and torch.equal(pb, pb2) and (m is None or torch.equal(m, m2))


# ------------------------------------------------------------------------------------------------- SGD + loss scale
@pytest.mark.parametrize("via_norm", [False, True])
def test_sgd_under_loss_scale_record_initialises_buffer_on_first_clean_step(via_norm):
    """overflow, clean, overflow, clean == two torch.optim.SGD steps on the clean gradients: the momentum buffer is
    initialised on the first step that is NOT skipped (t = step - scaler[5]), and the overflow calls leave p and the
    buffer untouched bit for bit.  found_inf comes from grad_scaler_check or from the norm pass."""
    o = ops()
    ref = torch.nn.Parameter(rnd(N, seed=1))
    opt = torch.optim.SGD([ref], lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-2)
    p = rnd(N, seed=1).to(DEV)
    buf = torch.full((N,), 123.0, device=DEV)             # garbage: the first clean step must overwrite, not read it
    rec = torch.tensor([1024.0, 0, 0, 0, 0, 0, 0, 0], device=DEV)
    state = torch.zeros(2, device=DEV)
    partials = torch.zeros(o.grad_norm_partials(N), dtype=torch.float64, device=DEV)
    clean = 0
    for call, overflow in enumerate((True, False, True, False)):
        scale = float(rec[0])
        gr = rnd(N, seed=20 + call)
        if not overflow:
            ref.grad = gr.clone()
            opt.step()
            clean += 1
        gs = (gr * scale).to(DEV)
        if overflow:
            gs[N - 1] = float("inf")
        before = (p.clone(), buf.clone())
        if via_norm:
            o.grad_norm(gs, N, state, partials, 1.0, rec, 1e3)
        else:
            o.grad_scaler_check(gs, N, rec)
        o.optim_step("sgd", p, gs, buf, None, None, N, 1e-3, 0.9, step=call + 1, scaler=rec, skip_slot=5,
                     weight_decay=1e-2, momentum=0.9, nesterov=True, norm_state=state if via_norm else None)
        o.grad_scaler_update(rec, 2.0, 0.5, 2000, skipped_ranges=2)
        torch.cuda.synchronize()
        if overflow:
            assert torch.equal(p, before[0]) and torch.equal(buf, before[1])
            assert float(rec[0]) == scale * 0.5
        assert float(rec[5]) == call + 1 - clean and float(rec[1]) == 0.0
    assert np.allclose(p.cpu().numpy(), ref.detach().numpy(), atol=1e-6, rtol=0)
    # the buffer holds 0.9 * g1 + g2 with |.| < 8 (ulp 9.5e-7); the kernel contracts into FMAs what torch rounds twice
    assert np.allclose(buf.cpu().numpy(), opt.state[ref]["momentum_buffer"].numpy(), atol=4e-6, rtol=0)


def test_optim_step_rejects_bad_arguments():
    o = ops()
    p = rnd(8).to(DEV)
    with pytest.raises(ValueError):
        o.optim_step("adamw", p, p, p, p, None, 8, 1e-3)
    with pytest.raises(RuntimeError, match="Nesterov"):
        o.optim_step("sgd", p, p, p, None, None, 8, 1e-3, momentum=0.9, dampening=0.1, nesterov=True)
    with pytest.raises(RuntimeError, match="buffer"):
        o.optim_step("sgd", p, p, None, None, None, 8, 1e-3, momentum=0.9)
    with pytest.raises(RuntimeError, match="partial"):
        o.grad_norm(rnd(2 ** 20).to(DEV), 2 ** 20, torch.zeros(2, device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV))
