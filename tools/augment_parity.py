#!/usr/bin/env python3
"""Measured errors of the device augmentation (csrc/augment.hip, csrc/reverb.hip, data/augment.py) next to their bounds:
runs tests/test_augment_gpu.py and tests/test_reverb_gpu.py (the tests print every figure before they assert) and keeps
the ``augment-parity:`` lines, in test order.  The output is what profiles/augment_parity.txt records.
    python tools/augment_parity.py [-o profiles/augment_parity.txt]"""
import argparse
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = ("# python tools/augment_parity.py on one MI355X: the lines tests/test_augment_gpu.py and tests/test_reverb_gpu.py print\n"
          "# before they assert.\n"
          "# Per case: the largest |device - float64 oracle| over the row, and the worst error / bound over its elements with\n"
          "# the per-element bounds of tests/augment_cases.py (FIR and resampler: (K + 2) 2^-24 sum_j |h_j x_j|, K the output's\n"
          "# live taps; mixes: 3 * 2^-24 (|c x| + |(1 - c) u|)).  Dropout, the copy ratio 1/1, the row-alone identity, the\n"
          "# untouched rows and guard bands and the uniform stream are bit-exact assertions and print no figure, except the\n"
          "# stream's own statistics.  The oracle is float64 numpy of the definitions in include/w2v2_hip.h.\n"
          "# Reverb lines (tests/reverb_cases.py): per row the largest |y_f64|, the largest error of the f32 SEQUENTIAL loop (sox's own\n"
          "# arithmetic, on the host) against float64, the device's, and the row's bound max(4 x the sequential loop's error,\n"
          "# 2^-22 max |y_f64|); dry gain 0 is the wet signal alone.\n")
TAG = "augment-parity: "


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None, help="write the lines here as well as to stdout")
    args = ap.parse_args()
    import pytest
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = pytest.main([os.path.join(ROOT, "tests", "test_augment_gpu.py"), os.path.join(ROOT, "tests", "test_reverb_gpu.py"), "-q", "-s",
                          "-m", "gpu", "-p", "no:cacheprovider"])
    lines = [ln[ln.index(TAG) + len(TAG):] for ln in buf.getvalue().splitlines() if TAG in ln]
    tail = buf.getvalue().strip().splitlines()[-1] if buf.getvalue().strip() else ""
    text = HEADER + "\n".join(lines) + f"\n# pytest: {tail.strip('= ')}\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
