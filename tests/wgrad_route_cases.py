"""Problem lists for the routing test of w2v2_wgrad_grouped (tests/test_host_cpu.py::test_wgrad_routing_table): what
``w2v2_wgrad_kernel_of`` answers needs no GPU (no device: the CU count falls back to 256) and no memory (the route reads
n_out / n_in only), so the operand pointers stay null.

Run as a script it prints the families of CASES as one JSON list, under whatever switches its environment carries and the
forced family named in ROUTE_FORCE; the test starts it in a fresh process per configuration because the library reads
its switches once."""
import json
import os
import sys


def block(H, I):
    """(n_out, n_in) of the four weight gradients of one transformer block: dW2, dW1, dWo, dWqkv."""
    return [(H, I), (I, H), (H, H), (3 * H, H)]


RES2NET = [(128, 384)] * 7          # the 128-channel dilated convolutions of one ECAPA Res2Net block (k = 3)
CASES = [  # (name, [(n_out, n_in), ...])
    ("base_block", block(768, 3072)), ("base_pair", block(768, 3072) * 2), ("base_four", block(768, 3072) * 4),
    ("large_block", block(1024, 4096)), ("large_pair", block(1024, 4096) * 2), ("large_four", block(1024, 4096) * 4),
    ("proj_slices", [(768, 512)] * 8), ("proj_slices_large", [(1024, 512)] * 8),
    ("ecapa_mix", RES2NET + [(1024, 1024), (1024, 1024), (128, 1024), (1024, 128)]), ("ecapa_res2net", RES2NET),
    ("ecapa_wide", [(1536, 3072), (3072, 1536)] + RES2NET), ("asp", [(768, 128), (128, 768)]),
    ("tiny_block", block(32, 64)), ("one_narrow", [(128, 768)]), ("one_small", [(64, 512)]), ("one_wide", [(136, 768)]),
    ("none", []), ("too_many", [(768, 768)] * 33),
]

CONFIGS = [  # (name, environment, forced family)
    ("default", {}, 0), ("wgrad_v1", {"W2V2_WGRAD_V1": "1"}, 0), ("no_wgrad4", {"W2V2_NO_WGRAD4": "1"}, 0),
    ("no_wgrad_ph", {"W2V2_NO_WGRAD_PH": "1"}, 0),
] + [(f"force_{f}", {}, f) for f in range(1, 7)]


def problems(_lib, sizes):
    arr = (_lib.WgradProblem * max(1, len(sizes)))()
    for q, (n_out, n_in) in zip(arr, sizes):
        q.n_out, q.n_in = n_out, n_in
    return arr


def families(force=0):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from w2v2_speaker_amd import _lib
    lib = _lib.load()
    lib.w2v2_tune_wgrad_kernel(force)
    return [lib.w2v2_wgrad_kernel_of(problems(_lib, sizes), len(sizes)) for _, sizes in CASES]


if __name__ == "__main__":
    print("ROUTE " + json.dumps(families(int(os.environ.get("ROUTE_FORCE", "0")))))
