"""Descriptors for the routing test of w2v2_gemm (tests/test_host_cpu.py::test_gemm_routing_table): what
``w2v2_gemm_kernel_of`` answers needs no GPU (no device: the CU count falls back to 256) and no real memory (the route
looks at pointer ALIGNMENT only), so the pointers below are made-up addresses.

Run as a script it prints the families of CASES as one JSON list, under whatever switches its environment carries and
the tuner calls named in ROUTE_TUNE ("kernel=2", "f32_tile=13"); the test starts it in a fresh process per configuration
because the library reads its switches once."""
import ctypes as C
import json
import os
import sys

F32, BF16, F16 = 0, 1, 2
STEP = [(9834, 768, 768), (9834, 2304, 768), (9834, 3072, 768), (9834, 768, 3072), (105534, 512, 1536), (66, 5994, 1536),
        (19800, 1024, 1024)]


def case(M, N, K, ab, c, **kw):
    return dict(M=M, N=N, K=K, ab=ab, c=c, **kw)


CASES = []
# the step's shapes: 16-bit and f32 outputs of both 16-bit formats, exact f32, two-term weights
for ab, c in ((F16, F16), (BF16, BF16), (F16, F32), (BF16, F32), (F32, F32)):
    CASES += [case(M, N, K, ab, c) for (M, N, K) in STEP]
CASES += [case(M, N, K, F16, F16, k_ext=K) for (M, N, K) in STEP]
CASES += [
    # transposed operands
    case(9834, 768, 768, F16, F16, ta=1), case(9834, 768, 768, F16, F16, tb=1), case(9834, 768, 768, F16, F32, ta=1, tb=1),
    case(9834, 3072, 768, BF16, BF16, tb=1), case(768, 3072, 9834, F16, F32, ta=1, tb=1),
    # split-K / accumulate
    case(9834, 768, 768, F16, F32, split=4), case(9834, 3072, 768, BF16, F32, split=2), case(9834, 768, 768, F16, F32, acc=1),
    case(1024, 1024, 19800, F32, F32, ta=1, tb=1, split=8), case(128, 384, 19800, F32, F32, ta=1, tb=1, split=32),
    case(9834, 768, 768, F16, F16, split=4),                                       # rejected: split-K needs an f32 C
    # a misaligned pointer / leading dimension
    case(9834, 768, 768, F16, F16, a_off=2), case(9834, 3072, 768, F16, F16, b_off=4), case(9834, 3072, 768, F16, F16, c_off=2),
    case(19800, 1024, 1024, F32, F32, a_off=4), case(9834, 768, 768, F16, F16, lda=772),
    # two-term weights: accepted and rejected
    case(9834, 2304, 768, F16, F16, k_ext=768, n_ext_from=768), case(9834, 2304, 768, BF16, F32, k_ext=768, n_ext_from=1536),
    case(66, 256, 768, F16, F16, k_ext=768),
    case(200, 136, 160, F16, F16, k_ext=160), case(9834, 2304, 768, F16, F16, k_ext=384),
    case(9834, 2304, 768, F16, F16, k_ext=768, n_ext_from=64), case(9834, 2304, 768, F16, F16, k_ext=768, tb=1),
    case(9834, 2304, 768, F16, F32, k_ext=768, split=2),
    # exact f32: eligible and ineligible for the LDS-DMA kernel
    case(19800, 1024, 1022, F32, F32), case(19800, 1024, 1024, F32, F32, tb=1), case(9834, 768, 768, F32, F32, ta=1),
    case(9832, 768, 768, F32, F32, ta=1), case(19800, 1022, 1024, F32, F32, tb=1), case(64, 1024, 1024, F32, F32),
    case(19800, 64, 384, F32, F32), case(19800, 128, 384, F32, F32), case(19800, 3072, 3072, F32, F32),
    case(19800, 1024, 1024, F32, F32, a_seg=(100, 1024 * 128)),
    # edges of the 16-bit rules
    case(9834, 64, 768, F16, F16), case(1000, 768, 768, F16, F16), case(1024, 512, 768, F16, F16), case(9834, 768, 96, F16, F16),
    case(9834, 768, 0, F16, F16), case(149, 149, 64, F16, F16, batch=792), case(9834, 3072, 768, F16, F16, batch=2),
    case(9834, 3000, 768, F16, F16), case(9834, 3072, 768, F16, F16, aux_off=2), case(9834, 3104, 768, F16, F16),
    case(3000000, 512, 1024, F16, F16), case(105534, 512, 1024, F16, F16, a_seg=(9594, 9600 * 512), lda=1024),
    case(316606, 512, 1536, BF16, BF16), case(9834, 1024, 1024, BF16, BF16), case(19668, 768, 768, F16, F16),
    # rejected descriptors
    case(0, 768, 768, F16, F16), case(9834, 768, 768, F16, BF16), case(9834, 768, 768, F32, F16),
]

CONFIGS = [  # (name, environment, tuner calls)
    ("default", {}, ""), ("no_gemm_ph", {"W2V2_NO_GEMM_PH": "1"}, ""), ("no_glds3", {"W2V2_NO_GLDS3": "1"}, ""),
    ("no_glds", {"W2V2_NO_GLDS": "1"}, ""), ("g3n_1024", {"W2V2_G3N": "1024"}, ""), ("f32_no_dma", {"W2V2_F32_NO_DMA": "1"}, ""),
    ("reserve_32", {"W2V2_RESERVE_CUS": "32"}, ""), ("kernel_1", {}, "kernel=1"), ("kernel_2", {}, "kernel=2"),
    ("kernel_4", {}, "kernel=4"), ("f32_tile_1", {}, "f32_tile=1"), ("f32_tile_13", {}, "f32_tile=13"),
]


def descriptor(_lib, cs):
    base = 0x7F0000000000
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.batch, d.batch_inner = cs["M"], cs["N"], cs["K"], cs.get("batch", 1), 1
    d.dtype_ab, d.dtype_c, d.epilogue = cs["ab"], cs["c"], 0
    ta, tb = cs.get("ta", 0), cs.get("tb", 0)
    d.A.ptr, d.A.trans, d.A.ld = base + cs.get("a_off", 0), ta, cs.get("lda", cs["M"] if ta else cs["K"])
    d.B.ptr, d.B.trans, d.B.ld = base + (1 << 36) + cs.get("b_off", 0), tb, cs["N"] if tb else cs["K"]
    if "a_seg" in cs:
        d.A.seg_len, d.A.seg_stride = cs["a_seg"]
    if d.batch > 1:
        d.A.stride0, d.B.stride0, d.c_stride0 = cs["M"] * cs["K"], cs["N"] * cs["K"], cs["M"] * cs["N"]
    d.C, d.ldc = base + (2 << 36) + cs.get("c_off", 0), cs["N"]
    if "aux_off" in cs:
        d.aux, d.ldaux, d.epilogue = base + (3 << 36) + cs["aux_off"], cs["N"], 4      # EPI_ADD
    d.alpha, d.split_k, d.accumulate = 1.0, cs.get("split", 1), cs.get("acc", 0)
    d.k_ext, d.n_ext_from, d.b_lo_offset = cs.get("k_ext", 0), cs.get("n_ext_from", 0), 8 * cs["N"] * cs["K"] * bool(cs.get("k_ext"))
    return d


def families(tune=""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from w2v2_speaker_amd import _lib
    lib = _lib.load()
    for call in filter(None, tune.split(",")):
        name, val = call.split("=")
        {"kernel": lib.w2v2_tune_gemm_kernel, "f32_tile": lib.w2v2_tune_gemm_f32_tile}[name](int(val))
    out = [lib.w2v2_gemm_kernel_of(C.byref(descriptor(_lib, cs))) for cs in CASES]
    assert lib.w2v2_gemm_f32_last_kernel() == 0          # the route launches nothing and records nothing
    return out


if __name__ == "__main__":
    print("ROUTE " + json.dumps(families(os.environ.get("ROUTE_TUNE", ""))))
