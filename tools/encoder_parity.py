#!/usr/bin/env python3
"""Measured errors of the layer-norm and fused-attention kernels (csrc/norm.hip, csrc/attention.hip) next to their bounds:
runs tests/test_encoder_cases_cpu.py and tests/test_encoder_kernels_gpu.py (the tests print every figure before they
assert) and keeps the ``encoder-parity:`` lines, in test order.  The output is what profiles/encoder_parity.txt records.
    python tools/encoder_parity.py [-o profiles/encoder_parity.txt]"""
import argparse
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = "encoder-parity: "
HEADER = (
    "# python tools/encoder_parity.py on one MI355X: the lines tests/test_encoder_cases_cpu.py and\n"
    "# tests/test_encoder_kernels_gpu.py print before they assert.  Every figure is the worst |device - float64 reference|\n"
    "# over the shapes of the case (the one closest to its bound, named in brackets) followed by that bound.\n"
    "#   layernorm fwd: |d mean| * rstd_ref and rel |d rstd| over the rows, bound 2^-22 + 8 x the same error of an f32\n"
    "#          two-pass on the f32 sum; y: rel-L2 of the worst row, bound u(dtype) + 2e-6 * max(1, rms_s * rstd) with\n"
    "#          u = 0 / 2^-8 / 2^-11 for f32 / bf16 / fp16; the stored sum x + r * mask is compared bit for bit.\n"
    "#   layernorm bwd: ds and d_r as rel-L2 of the worst row, bound u(dtype) + 1e-5; dgamma / dbeta as the worst column's\n"
    "#          |error| / sum of the |terms| (the pre-filled value is one of them), bound 2e-5.  M runs up to 2 * 4 * cap + 5.\n"
    "#   layernorm chained: |x-hat rebuilt from the stored 16-bit sum - x-hat of the unrounded sum| per element, bound\n"
    "#          u(dtype) * |s| * rstd plus what the statistics bound allows.\n"
    "#   attention: rel-L2 of the worst 64-element row of ctx / dq / dk / dv, bound 2 x the error of the ideal 16-bit\n"
    "#          attention (float64 with the kernel's documented roundings; the backward at three f32 roundings of the\n"
    "#          exponent, the largest error counts) ON THAT ROW + 2e-6; 'kernel/yardstick' is the worst\n"
    "#          row's ratio of the two errors (each over the f32 term as well), so the bound is met exactly when it is <= 2.\n"
    "#          dq / dk of `peaked` (and wherever dS is exactly zero) are absolute, on rms(dctx) rms(v) rms(k) scale.\n"
    "#          lse: max |error|, bound 2^-22 max(1, |lse|) + 8 x an f32 CPU evaluation's error; delta: |error| / sum |dO ctx|,\n"
    "#          bound 2e-6.\n"
    "#   '(bit-equal)' is 0 when the two sides are identical and inf otherwise.\n")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None, help="write the lines here as well as to stdout")
    args = ap.parse_args()
    import pytest
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = pytest.main([os.path.join(ROOT, "tests", "test_encoder_cases_cpu.py"),
                          os.path.join(ROOT, "tests", "test_encoder_kernels_gpu.py"),
                          "-q", "-s", "-m", "gpu or not gpu", "-p", "no:cacheprovider"])
    lines = [ln[ln.index(MARK) + len(MARK):] for ln in buf.getvalue().splitlines() if MARK in ln]
    tail = buf.getvalue().strip().splitlines()[-1] if buf.getvalue().strip() else ""
    text = HEADER + "\n".join(lines) + f"\n# pytest: {tail.strip('= ')}\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
