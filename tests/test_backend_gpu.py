"""LDA / PLDA scoring back-ends on the GPU: the three kernels of csrc/backend.hip and ops.class_scatter on the cases and
within the bounds of tests/backend_cases.py (NaN-filled row gaps, sentinels behind every output, every kernel twice for
equal bits), the device fit and scoring of the two evaluators against the all-float64 oracle, and a module whose
evaluator is a PLDAEvaluator.  Every ``backend-parity:`` line goes to profiles/backend_parity.txt."""
import numpy as np
import pytest
import torch

import backend_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 12345.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gapped(a, gap=4):
    """[rows, D] numpy -> a device view [rows, D] with row stride D + gap, NaN in the gap."""
    buf = np.full((a.shape[0], a.shape[1] + gap), np.nan, dtype=a.dtype)
    buf[:, :a.shape[1]] = a
    return dev(buf)[:, :a.shape[1]]


# ------------------------------------------------------------------------------------------------ rows_center
@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("rows", (1, 7, 300))
@pytest.mark.parametrize("D", (4, 8, 132))
def test_rows_center_bit_equal_to_numpy(D, rows, S):
    from w2v2_speaker_amd import ops
    rng = np.random.default_rng(100 * D + rows + S)
    x = (rng.standard_normal((rows, D)) * 2 + 1).astype(np.float32)
    means = rng.standard_normal((S, D)).astype(np.float32)
    seg = rng.integers(0, S, rows).astype(np.int32)
    w = (rng.random(rows) * 3).astype(np.float32)
    for use_seg in (False, True):
        for use_w in (False, True):
            want = bc.rows_center_reference(x, means, seg if use_seg else None, w if use_w else None)
            runs = []
            for _ in range(2):
                out = torch.full((rows + 1, D + 4), SENTINEL, dtype=torch.float32, device=DEV)
                got = ops.rows_center(gapped(x), gapped(means), dev(seg) if use_seg else None, dev(w) if use_w else None,
                                      out=out[:rows, :D])
                assert got.data_ptr() == out.data_ptr()
                runs.append(out.cpu().numpy())
            assert np.array_equal(runs[0], runs[1])
            assert (runs[0][rows:] == SENTINEL).all() and (runs[0][:, D:] == SENTINEL).all(), "written outside the output"
            assert np.array_equal(runs[0][:rows, :D].view(np.uint32), want.view(np.uint32)), (use_seg, use_w)


@pytest.mark.parametrize("D", (4, 132))
def test_rows_center_a_bad_segment_poisons_its_own_row_only(D):
    from w2v2_speaker_amd import ops
    rng = np.random.default_rng(D)
    rows, S = 7, 3
    x, means = rng.standard_normal((rows, D)).astype(np.float32), rng.standard_normal((S, D)).astype(np.float32)
    seg = rng.integers(0, S, rows).astype(np.int32)
    seg[2], seg[5] = -1, S
    want = bc.rows_center_reference(x, means, seg, None)
    out = torch.full((rows + 1, D + 4), SENTINEL, dtype=torch.float32, device=DEV)
    ops.rows_center(gapped(x), gapped(means), dev(seg), None, out=out[:rows, :D])
    got = out.cpu().numpy()
    assert np.isnan(got[[2, 5], :D]).all() and (got[:, D:] == SENTINEL).all() and (got[rows:] == SENTINEL).all()
    keep = [0, 1, 3, 4, 6]
    assert np.array_equal(got[keep, :D], want[keep])


def test_scatter_fold_first_overwrites_and_later_calls_add():
    from w2v2_speaker_amd import ops
    rng = np.random.default_rng(3)
    for D in (4, 36, 132):
        blocks = [rng.standard_normal((D, D)).astype(np.float32) * 1e3 for _ in range(3)]
        acc = torch.full((D * D + 2,), float("nan"), dtype=torch.float64, device=DEV)
        acc[D * D:] = SENTINEL
        view = acc[:D * D].view(D, D)
        for i, b in enumerate(blocks):
            ops.scatter_fold(gapped(b), view, first=i == 0)
        got = acc.cpu().numpy()
        want = (blocks[0].astype(np.float64) + blocks[1]) + blocks[2]
        assert np.array_equal(got[:D * D].reshape(D, D), want) and (got[D * D:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ class_scatter
@pytest.mark.parametrize("N,rpb", ((5, 256), (257, 256), (1030, 256), (100, 4096)))
@pytest.mark.parametrize("D", (4, 36, 132))
def test_class_scatter_within_the_fma_chain_bound(D, N, rpb):
    from w2v2_speaker_amd import ops
    rng = np.random.default_rng(1000 * D + N)
    bank, ids, C = bc.scatter_case(rng, N, D, 256)
    counts = np.bincount(ids, minlength=C)
    assert N < 100 or (counts.min() == 1 and (N <= 512 or counts.max() >= 256))
    means = np.stack([bank[ids == c].astype(np.float64).mean(axis=0) for c in range(C)]).astype(np.float32)
    mu0 = bank.astype(np.float64).mean(axis=0).astype(np.float32)[None]
    root_n = np.sqrt(counts).astype(np.float32)
    work = torch.full((ops.class_scatter_workspace(N, D, rpb) + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    cases = (("S_w", bank, ids, means, None), ("S_b", means, None, mu0, root_n))
    for name, rows, seg, mean_rows, weight in cases:
        a = bc.rows_center_reference(rows, mean_rows, seg, weight)
        want, bound = bc.scatter_reference(a, min(rpb, len(rows)))
        runs = [ops.class_scatter(gapped(rows), None if seg is None else dev(seg), gapped(mean_rows),
                                  None if weight is None else dev(weight), rows_per_block=rpb, workspace=work).cpu().numpy()
                for _ in range(2)]
        assert np.array_equal(runs[0], runs[1])
        assert (work[-4:] == SENTINEL).all(), "written past the workspace"
        err = np.abs(runs[0] - want)
        print(f"backend-parity: class_scatter {name} N={len(rows)} D={D} rows_per_block={rpb}: max err / bound "
              f"{(err / np.maximum(bound, 1e-300)).max():.3f} (bound (rows_per_block + 4) 2^-24 sum |a_ri||a_rj|), max err "
              f"{err.max():.2e} at |S| max {np.abs(want).max():.2e}")
        assert (err <= bound).all(), name


# ------------------------------------------------------------------------------------------------ plda_score_pairs
@pytest.mark.parametrize("P", (1, 65, 1000))
@pytest.mark.parametrize("Q", (4, 12, 200))
def test_plda_score_pairs_against_float64(Q, P):
    from w2v2_speaker_amd import ops
    rng = np.random.default_rng(10 * Q + P)
    N = 37
    u = (rng.standard_normal((N, Q)) * 1.5).astype(np.float32)
    psi = np.sort(rng.random(Q) * 20)[::-1].copy()
    psi[0], psi[-1] = 1e4, 0.0
    p, q, k = bc.coefficients(psi)
    pairs = rng.integers(0, N, (P, 2)).astype(np.int32)
    pairs[0] = (5, 5)                                        # a row with itself
    want, mag = bc.llr_closed_form(u[pairs[:, 0]], u[pairs[:, 1]], p, q, k)
    bound = 2.0 ** -24 * np.abs(want) + Q * 2.0 ** -52 * mag
    runs = []
    for _ in range(2):
        out = torch.full((P + 4,), SENTINEL, dtype=torch.float32, device=DEV)
        ops.plda_score_pairs(gapped(u), dev(pairs), dev(p), dev(q), k, out)
        runs.append(out.cpu().numpy())
    assert np.array_equal(runs[0], runs[1]) and (runs[0][P:] == SENTINEL).all()
    err = np.abs(runs[0][:P].astype(np.float64) - want)
    print(f"backend-parity: plda_score_pairs Q={Q} P={P}: max err / bound {(err / bound).max():.3f} "
          f"(bound 2^-24 |llr| + Q 2^-52 sum |terms|), |llr| max {np.abs(want).max():.2e}")
    assert (err <= bound).all()


def test_plda_score_pairs_a_bad_index_poisons_its_own_trial_only():
    from w2v2_speaker_amd import ops
    rng = np.random.default_rng(9)
    N, Q = 11, 12
    u = rng.standard_normal((N, Q)).astype(np.float32)
    p, q, k = bc.coefficients(np.linspace(5, 0.1, Q))
    pairs = rng.integers(0, N, (9, 2)).astype(np.int32)
    clean = ops.plda_score_pairs(gapped(u), dev(pairs), dev(p), dev(q), k).cpu().numpy()
    pairs[3, 0], pairs[6, 1] = -1, N
    got = ops.plda_score_pairs(gapped(u), dev(pairs), dev(p), dev(q), k).cpu().numpy()
    keep = [0, 1, 2, 4, 5, 7, 8]
    assert np.isnan(got[[3, 6]]).all() and np.array_equal(got[keep], clean[keep])


def test_host_checks_raise_before_any_launch():
    from w2v2_speaker_amd import ops
    x, m = torch.zeros(8, 8, device=DEV), torch.zeros(2, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.rows_center(torch.zeros(8, 6, device=DEV), torch.zeros(2, 6, device=DEV))
    with pytest.raises(ValueError):
        ops.rows_center(x, torch.zeros(2, 12, device=DEV))
    with pytest.raises(ValueError):
        ops.rows_center(x, m, seg_id=torch.zeros(8, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ops.rows_center(x, m, out=x)
    with pytest.raises(ValueError):
        ops.scatter_fold(x, torch.zeros(8, 8, device=DEV), True)
    with pytest.raises(ValueError):
        ops.class_scatter(x, None, m, rows_per_block=0)
    with pytest.raises(ValueError):
        ops.class_scatter(x, None, m, workspace=torch.zeros(8, device=DEV))
    with pytest.raises(ValueError):
        ops.plda_score_pairs(x, torch.zeros(3, 2, dtype=torch.int32, device=DEV), torch.zeros(8, device=DEV),
                             torch.zeros(8, device=DEV), 0.0)
    lib = ops.lib()
    assert lib.w2v2_rows_center(x.data_ptr(), 8, 8, 8, None, m.data_ptr(), 8, 0, None, x.data_ptr(), 8, None) != 0
    assert b"rows_center" in lib.w2v2_last_error()
    assert lib.w2v2_scatter_fold(x.data_ptr(), 8, None, 8, 1, None) != 0
    assert lib.w2v2_plda_score_pairs(x.data_ptr(), 8, 8, 6, x.data_ptr(), 1, x.data_ptr(), x.data_ptr(), 0.0, x.data_ptr(), None) != 0


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def e2e():
    train, labels, test, test_labels, pairs, gt = bc.two_covariance_set(0, **bc.E2E)
    from w2v2_speaker_amd.evaluation.speaker import EvaluationPair
    keys = [f"u{r}" for r in range(len(test))]
    trial = [EvaluationPair(bool(g), keys[i], keys[j]) for (i, j), g in zip(pairs.tolist(), gt)]
    return dict(train=train, labels=labels, test=test, pairs=pairs, gt=gt, keys=keys, trial=trial, oracle={})


def _oracle(e2e, kind, projection):
    """(float64 scores, distance of the f32 numpy pipeline from them), computed once per back-end."""
    if (kind, projection) not in e2e["oracle"]:
        kw = dict(kind=kind, projection_kind=projection, R=bc.E2E["R"], Q=bc.E2E["Q"], iterations=bc.E2E["iterations"])
        s64 = bc.fit_and_score(e2e["train"], e2e["labels"], e2e["test"], e2e["pairs"], **kw)
        s32 = bc.fit_and_score(e2e["train"], e2e["labels"], e2e["test"], e2e["pairs"], work=np.float32, **kw)
        if kind == "lda":                                    # what the evaluator feeds the metrics: (cos + 1) / 2, clipped
            s64, s32 = np.clip((s64 + 1) / 2, 0, 1), np.clip((s32 + 1) / 2, 0, 1)
        e2e["oracle"][kind, projection] = (s64, float(np.abs(s32 - s64).max()))
    return e2e["oracle"][kind, projection]


@pytest.mark.parametrize("metrics", ("host", "device"))
@pytest.mark.parametrize("kind,projection", (("lda", "pca"), ("lda", "lda"), ("plda", "pca"), ("plda", "lda")))
def test_device_fit_and_scoring_against_the_float64_oracle(e2e, kind, projection, metrics):
    from w2v2_speaker_amd.evaluation.speaker import LDAEvaluator, PLDAEvaluator
    from w2v2_speaker_amd.eval_metrics import calculate_eer
    R, Q, its = bc.E2E["R"], bc.E2E["Q"], bc.E2E["iterations"]
    ev = LDAEvaluator(True, True, 0, R, False, projection=projection) if kind == "lda" \
        else PLDAEvaluator(R, Q, its, 0, projection=projection)
    ev.fit_parameters_bank(gapped(e2e["train"]), e2e["labels"])
    res = ev.evaluate_bank_metrics(e2e["trial"], e2e["keys"], gapped(e2e["test"]), metrics=metrics)
    rec = ev.last_bank_scoring
    P = len(e2e["pairs"])
    if metrics == "device":
        assert rec.scores is None and rec.host_copy_floats == 0 and ev.last_bank_metrics.path == "device"
        got = rec.device_scores.cpu().numpy().astype(np.float64)
    else:
        assert rec.host_copy_floats == P
        got = rec.scores
    want, f32_err = _oracle(e2e, kind, projection)
    err = float(np.abs(got - want).max())
    print(f"backend-parity: {kind} projection={projection} metrics={metrics} D=32 R=Q=16 {its} EM steps, {P} trials: device vs "
          f"float64 {err:.2e}, f32 numpy pipeline vs float64 {f32_err:.2e}, ratio {err / f32_err:.2f} (allowed "
          f"{bc.DEVICE_MARGIN:.0f}), |score| max {np.abs(want).max():.2e}, eer {res['eer']:.4f}")
    assert err <= bc.DEVICE_MARGIN * f32_err
    host_eer = calculate_eer(e2e["gt"], got.tolist(), pos_label=1)[0]
    assert abs(res["eer"] - host_eer) <= 1e-3
    if kind == "plda" and projection == "pca":               # a condition, not a measurement
        cos_eer = calculate_eer(e2e["gt"], bc.cosine_scores(e2e["test"], e2e["pairs"]).tolist(), pos_label=1)[0]
        print(f"backend-parity: plda eer {res['eer']:.4f} against the plain cosine of the raw test bank {cos_eer:.4f}: ratio "
              f"{res['eer'] / cos_eer:.2f} (at most {bc.EER_RATIO})")
        assert res["eer"] <= bc.EER_RATIO * cos_eer


def test_device_fit_agrees_with_the_host_fit(e2e):
    """The two fits differ only in who summed the statistics: the fitted evaluators score alike on the host path."""
    from w2v2_speaker_amd.evaluation.speaker import EmbeddingSample, PLDAEvaluator
    a, b = PLDAEvaluator(14, 6, 3, 0), PLDAEvaluator(14, 6, 3, 0)
    a.fit_parameters_bank(dev(e2e["train"]), e2e["labels"])
    b.fit_parameters([torch.from_numpy(e2e["train"])], [torch.tensor(e2e["labels"])])
    samples = [EmbeddingSample(k, torch.from_numpy(e2e["test"][r])) for r, k in enumerate(e2e["keys"])]
    ra, rb = a.evaluate(e2e["trial"], samples), b.evaluate(e2e["trial"], samples)
    assert abs(ra["eer"] - rb["eer"]) <= 1e-2               # (one of the 240 target trials moves the miss rate by 4e-3)
    np.testing.assert_allclose(a.psi.numpy(), b.psi.numpy(), rtol=1e-3)
    np.testing.assert_allclose(a._k, b._k, rtol=1e-3)


def test_lda_center_before_fit_and_score_norm_on_the_device(e2e):
    from w2v2_speaker_amd.evaluation.speaker import EmbeddingSample, LDAEvaluator
    from w2v2_speaker_amd.evaluation.speaker.device_scoring import ScoreNorm, speaker_mean_cohort
    ev = LDAEvaluator(True, True, 0, 16, True, projection="lda")
    train = dev(e2e["train"])
    ev.fit_parameters_bank(train, e2e["labels"])
    sn = ScoreNorm(speaker_mean_cohort(train, e2e["labels"]), 10, "s")
    got = ev.evaluate_bank_metrics(e2e["trial"], e2e["keys"], dev(e2e["test"]), score_norm=sn)
    scores = ev.last_bank_scoring.scores
    samples = [EmbeddingSample(k, torch.from_numpy(e2e["test"][r])) for r, k in enumerate(e2e["keys"])]
    sn_host = ScoreNorm(sn.cohort.cpu(), 10, "s")
    host = ev.evaluate(e2e["trial"], samples, score_norm=sn_host)
    assert np.abs(scores).max() > 1.5 and abs(got["eer"] - host["eer"]) <= 1e-2
    # the same fitted model on both paths: only the f32 order of operations differs
    pairs = torch.from_numpy(e2e["pairs"].astype(np.int64))
    host_scores = ev._host_scores(ev._host_latent(torch.from_numpy(e2e["test"])), pairs[:, 0], pairs[:, 1], sn_host).numpy()
    assert np.abs(scores - host_scores).max() <= 1e-3 * np.abs(host_scores).max()


def test_module_with_a_plda_evaluator_scores_like_the_evaluator_itself(e2e):
    import test_varlen_ecapa_gpu as VE
    from w2v2_speaker_amd.evaluation.speaker import EvaluationPair, PLDAEvaluator
    from w2v2_speaker_amd.lightning_modules.speaker.ecapa_tdnn import EcapaTDNNModuleConfig, EcapaTdnnModule
    c = VE.E.EcapaConfig.tiny()
    mcfg = EcapaTDNNModuleConfig(input_mel_coefficients=c.input_size, lin_neurons=c.lin_neurons, channels=list(c.channels),
                                 kernel_sizes=list(c.kernel_sizes), dilations=list(c.dilations),
                                 attention_channels=c.attention_channels, res2net_scale=c.res2net_scale,
                                 se_channels=c.se_channels)
    ev = PLDAEvaluator(8, 8, 2, 0)
    mod = EcapaTdnnModule.from_config(mcfg, num_speakers=6, device=DEV, act_dtype=torch.float32, evaluator=ev)
    mod.store.load_state_dict(VE.E.make_state_dict(c, 20211), strict=False)
    for n, r in mod.store.bn_running.items():
        r.copy_(VE._running(n, r.numel() // 2).to(DEV))
    assert mod.evaluator is ev
    lens, kw = (20, 130, 390), dict(quantum=50, max_batch_frames=4 * 400, max_batch=4)
    inputs = {f"u{i}": torch.randn(lens[i % 3], c.input_size, generator=torch.Generator().manual_seed(i)) for i in range(6)}
    keys = sorted(inputs)
    bank = torch.cat(mod.compute_speaker_embeddings([inputs[k] for k in keys], **kw)).detach().float()
    # a training bank around the module's own embeddings: 12 speakers x 5
    rng = np.random.default_rng(4)
    centre, spread = bank.cpu().numpy().mean(axis=0), bank.cpu().numpy().std() + 1e-3
    spk = centre + spread * rng.standard_normal((12, bank.shape[1]))
    train = (np.repeat(spk, 5, axis=0) + 0.5 * spread * rng.standard_normal((60, bank.shape[1]))).astype(np.float32)
    ev.fit_parameters_bank(dev(train), [i // 5 for i in range(60)])
    idx = [(i, j) for i in range(6) for j in range(i + 1, 6)]
    pairs = [EvaluationPair(bool((i + j) % 3 == 0 or j == i + 1), keys[i], keys[j]) for i, j in idx]
    got = mod.evaluate_trials(pairs, inputs, scoring="device", metrics="device", **kw)
    scores = ev.last_bank_scoring.device_scores.cpu().numpy()
    direct = ev.evaluate_bank_metrics(pairs, keys, bank, metrics="device")
    assert got == direct and np.array_equal(scores, ev.last_bank_scoring.device_scores.cpu().numpy())
    assert np.isfinite(scores).all() and set(got) == {"eer", "eer_threshold", "mdc", "mdc_threshold"}
