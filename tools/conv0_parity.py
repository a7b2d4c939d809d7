#!/usr/bin/env python3
"""Measured errors of the conv feature-extractor kernels (csrc/conv0.hip) next to their bounds: runs
tests/test_conv0_cpu.py and tests/test_conv0_gpu.py (the tests print every figure before they assert) and keeps the
``conv0-parity:`` lines, in test order.  The output is what profiles/conv0_parity.txt records.
    python tools/conv0_parity.py [-o profiles/conv0_parity.txt]"""
import argparse
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = "conv0-parity: "
HEADER = ("# python tools/conv0_parity.py on one MI355X: the lines tests/test_conv0_cpu.py and tests/test_conv0_gpu.py print\n"
          "# before they assert.  Per case family, dtype, width and input class: the worst |device - float64 reference| over\n"
          "# the lengths of the case (the one closest to its bound, named in brackets) and that bound.\n"
          "#   stats: max over (b, c) of |d mean| * rstd_ref and of rel |d rstd|; bound 2^-22 + 8 x the same error of an ideal\n"
          "#          f32 statistics pass (f32 FMA-chain convolution, float64 moments), a property of the inputs alone.\n"
          "#   apply: rel-L2 of the worst frame (over its channels) and of the worst channel (over its frames);\n"
          "#          f32 bound 2e-6 * max(1, rms_u / sd_u), 16-bit bound 4e-3; one frame (var = 0): |error| over the\n"
          "#          absolute bound of conv0_cases.degenerate_abs_bound, bound 1.\n"
          "#   bwd:   dw as max |error| / sum of the |terms| of the cancelling sum, dgamma / dbeta rel-L2, bound 2e-5.\n"
          "#   '(bit-equal)' is 0 when the two sides are identical and inf otherwise.\n")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None, help="write the lines here as well as to stdout")
    args = ap.parse_args()
    import pytest
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = pytest.main([os.path.join(ROOT, "tests", "test_conv0_cpu.py"),
                          os.path.join(ROOT, "tests", "test_conv0_gpu.py"),
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
