#!/usr/bin/env python3
"""Measured errors of the ECAPA-TDNN backward stages next to their bounds: runs tests/test_ecapa_stages_cpu.py and
tests/test_ecapa_stages_gpu.py (the tests print every figure before they assert) and keeps the ``ecapa-stage-parity:``
lines, in test order.  The output is what profiles/ecapa_stage_parity.txt records.
    python tools/ecapa_stage_parity.py [-o profiles/ecapa_stage_parity.txt]"""
import argparse
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = "ecapa-stage-parity: "
HEADER = ("# python tools/ecapa_stage_parity.py on one MI355X: the lines tests/test_ecapa_stages_cpu.py and\n"
          "# tests/test_ecapa_stages_gpu.py print before they assert.  Per geometry, dtype, training step and stage kind: the\n"
          "# worst |device - float64 reference of the stage's own stored operands| over all blocks (the one closest to its\n"
          "# bound, named in brackets), the rounding floor of that reference in the stored dtype, and the bound\n"
          "# 2 * r * floor + 2e-5.  rel-L2 unless marked: '/sum|terms|' is max |error| / sum of the |terms| of a cancelling sum,\n"
          "# '(bit-equal)' is 0 when the two sides are identical and inf otherwise.\n")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None, help="write the lines here as well as to stdout")
    args = ap.parse_args()
    import pytest
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = pytest.main([os.path.join(ROOT, "tests", "test_ecapa_stages_cpu.py"),
                          os.path.join(ROOT, "tests", "test_ecapa_stages_gpu.py"),
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
