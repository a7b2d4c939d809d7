"""The float64 stage references of tests/ecapa_stage_cases.py are themselves right: chained in the plan's order over an
f64 forward of oracle/ecapa_oracle.py they give the gradients torch autograd gives for ``ecapa_forward``.  The device
tests (tests/test_ecapa_stages_gpu.py) hold every kernel stage to these references, this test holds the references to
the oracle the goldens pin.  No GPU."""
import torch

import ecapa_stage_cases as K
from oracle import ecapa_oracle as E


def test_chained_stage_references_equal_autograd_of_the_oracle_in_f64():
    """EcapaConfig.tiny(), B = 3, T = 37, a random gradient at the MFA output: every TDNN, BatchNorm and SE parameter
    gradient and the gradient wrt the features, hand-written chain against autograd, both in f64 -- the same formulas in
    another summation order, so the bound is 1e-10 rel-L2."""
    cfg = E.EcapaConfig.tiny()
    assert (cfg.kernel_sizes, cfg.dilations) == (K.KERNEL_SIZES, K.DILATIONS)
    g = torch.Generator().manual_seed(7)
    B, T = 3, 37
    feat = torch.randn(B, T, cfg.input_size, generator=g, dtype=K.F64)
    sd = {n: v.to(K.F64) for n, v in E.make_state_dict(cfg, 20211).items()}
    up = torch.randn(B, T, cfg.channels[-1], generator=g, dtype=K.F64)

    sdg = {n: v.clone().requires_grad_(True) for n, v in sd.items()}
    fr = feat.clone().requires_grad_(True)
    _, stages = E.ecapa_forward(fr, sdg, cfg, return_stages=True)
    (stages["mfa"] * up).sum().backward()

    with torch.no_grad():
        rec, mfa = K.forward_record(feat, sd, cfg)
    assert K.rel_l2(mfa, stages["mfa"].detach()) < 1e-12            # the record IS the oracle's forward
    grads, d_feat = K.chain_backward(rec, sd, cfg, up.reshape(B * T, -1))

    worst = {}
    for n, v in sdg.items():
        if n.startswith(("asp", "fc.")):                            # behind the MFA output: no gradient from this loss
            assert v.grad is None and n not in grads
            continue
        assert n in grads, n
        worst[n] = K.rel_l2(grads[n].reshape(v.shape), v.grad)
    worst["feat"] = K.rel_l2(d_feat.reshape(B, T, -1), fr.grad)
    assert len(worst) == len(grads) + 1
    bad = {n: e for n, e in worst.items() if not e < 1e-10}
    print(f"ecapa-stage-parity: cpu chain vs autograd (f64): worst rel-L2 {max(worst.values()):.2e} over {len(worst)} "
          f"gradients, bound 1.0e-10")
    assert not bad, bad
