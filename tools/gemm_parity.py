#!/usr/bin/env python3
"""Measured errors of the w2v2_gemm kernel families (csrc/gemm*.hip) next to their bounds: runs the cases of
tests/gemm_cases.py through tests/test_gemm_cases_cpu.py and tests/test_gemm_edges_gpu.py (the tests print every figure
before they assert) and keeps the ``gemm-parity:`` lines, in test order.  The output is what profiles/gemm_parity.txt
records.
    python tools/gemm_parity.py [-o profiles/gemm_parity.txt]"""
import argparse
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = ("# python tools/gemm_parity.py on one MI355X: the lines tests/test_gemm_cases_cpu.py and tests/test_gemm_edges_gpu.py\n"
          "# print before they assert.  Per group of cases, operand > output type, kernel family and operand class: the\n"
          "# largest |device - float64 reference| over its per-element bound, over every element of every launch (real class:\n"
          "# nterms * 2^-24 * S + u_out * |ref|; gelu class: (0.75e-7 + 2 E) * max(1, |x|) + u_out * |ref|; tests/gemm_cases.py),\n"
          "# or, exact class, the number of launches that were bit-equal to the reference.  A 16-bit output sits near 1 by\n"
          "# construction: its bound is one rounding to nearest of the type, which the worst element of a matrix reaches.\n"
          "# The 'cpu' lines are torch's own f32 arithmetic on the CPU held to the same bounds.\n")
TAG = "gemm-parity: "


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None, help="write the lines here as well as to stdout")
    args = ap.parse_args()
    import pytest
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = pytest.main([os.path.join(ROOT, "tests", "test_gemm_cases_cpu.py"), os.path.join(ROOT, "tests", "test_gemm_edges_gpu.py"),
                          "-q", "-s", "-m", "gpu or not gpu", "-p", "no:cacheprovider"])
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
