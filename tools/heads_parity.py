#!/usr/bin/env python3
"""Measured errors of the loss-head kernels (csrc/heads.hip) next to their bounds: runs the cases of tests/heads_cases.py
through tests/test_heads_cpu.py and tests/test_heads_gpu.py (the tests print every figure before they assert) and keeps
the ``heads-parity:`` lines, in test order.  The output is what profiles/heads_parity.txt records.
    python tools/heads_parity.py [-o profiles/heads_parity.txt]"""
import argparse
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = ("# python tools/heads_parity.py on one MI355X: the lines tests/test_heads_cpu.py and tests/test_heads_gpu.py print\n"
          "# before they assert.  Each figure is |device - float64 reference| in the measure named (loss: relative to\n"
          "# max(1, |ref|); softmax / prob / dlogit: absolute; everything else: rel-L2, per row for the row kernel), followed by\n"
          "# its bound.\n")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None, help="write the lines here as well as to stdout")
    args = ap.parse_args()
    import pytest
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = pytest.main([os.path.join(ROOT, "tests", "test_heads_cpu.py"), os.path.join(ROOT, "tests", "test_heads_gpu.py"),
                          "-q", "-s", "-m", "gpu or not gpu", "-p", "no:cacheprovider"])
    lines = [ln[ln.index("heads-parity: ") + len("heads-parity: "):] for ln in buf.getvalue().splitlines()
             if "heads-parity: " in ln]
    tail = buf.getvalue().strip().splitlines()[-1] if buf.getvalue().strip() else ""
    text = HEADER + "\n".join(lines) + f"\n# pytest: {tail.strip('= ')}\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
