"""bench.py's own surface: --dump-outputs (what the timed path computed, float32, bounded) and the plain run (the headline
line and nothing that needs a pass of its own; everything else is behind --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_dump_outputs_writes_float32_within_budget(tmp_path):
    import bench
    flat = torch.arange(3 * bench.DUMP_WEIGHT_SAMPLE, dtype=torch.float32)
    big = torch.randn(bench.DUMP_MAX_ELEMENTS + 7, dtype=torch.float16)
    emb = torch.randn(4, 6, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), torch.tensor(1.5), big, emb, flat)
    bench.dump_outputs(str(tmp_path / "b"), torch.tensor(1.5), big, emb, flat)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["embedding.npy", "loss.npy", "softmax.npy", "weights_sample.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b), n          # fixed, seeded samples
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [1.5]
    assert np.array_equal(np.load(tmp_path / "a" / "embedding.npy"), emb.float().numpy())
    assert np.load(tmp_path / "a" / "softmax.npy").shape == (bench.DUMP_MAX_ELEMENTS,)
    w = np.load(tmp_path / "a" / "weights_sample.npy")
    assert w.shape == (bench.DUMP_WEIGHT_SAMPLE,) and np.all(np.diff(w) >= 0) and w.max() < flat.numel()


def test_bench_flags_default_to_a_plain_run():
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"]
        a = bench.parse_args()
        assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 2 and a.dtype == "f16"
        sys.argv = ["bench.py", "--full", "--dump-outputs", "d", "--model", "ecapa"]
        a = bench.parse_args()
        assert a.full is True and a.dump_outputs == "d" and a.dtype == "f32"
    finally:
        sys.argv = argv


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run with --dump-outputs: the contract fields, the requested number of timed steps, no side leg, and the
    last step's loss / softmax / embeddings / weight sample as finite float32 arrays -- the same bits in a second run
    with the same arguments (seeded inputs, no order-dependent reductions on the timed path)."""
    def run(out):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        return json.loads(lines[0])
    out = tmp_path / "dump"
    d = run(out)
    assert d["unit"] == "utterances/sec" and d["higher_is_better"] is True and d["dtype"] == "f16" and d["steps"] == 3
    assert abs(d["value"] - 66 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    for k in ("also", "eer", "roofline", "roofline_families", "cpu_baseline", "ms_per_step_median"):
        assert k not in d, k
    loss = np.load(out / "loss.npy")
    assert loss.dtype == np.float32 and abs(float(loss[0]) - d["config"]["final_loss"]) < 1e-3
    sm = np.load(out / "softmax.npy")
    assert sm.shape == (66, 5994) and np.allclose(sm.sum(axis=1), 1.0, atol=1e-3)
    assert np.load(out / "embedding.npy").shape == (66, 2 * 768)
    for n in ("softmax", "embedding", "weights_sample"):
        a = np.load(out / f"{n}.npy")
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
    # the default workload has no order-dependent reduction on its path (Determinism): a second run with the
    # same arguments must give the same bits; a difference names the array and its size
    run(tmp_path / "again")
    for n in ("loss", "softmax", "embedding", "weights_sample"):
        a, b = np.load(out / f"{n}.npy"), np.load(tmp_path / "again" / f"{n}.npy")
        assert np.array_equal(a, b), (n, float(np.abs(a.astype(np.float64) - b).max()), int((a != b).sum()))
