"""Build libw2v2hip.so (gfx950) in-tree with hipcc.  Used by ``__graft_entry__.build()`` and by the
loader when the library is missing and a compiler is present.  No fallback of any kind: if the build
fails the product path raises."""
from __future__ import annotations

import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libw2v2hip.so")
SOURCES = ["api.hip", "gemm.hip", "gemm_ring.hip", "gemm_phased.hip", "gemm_f32.hip", "gemm_f32_dma.hip", "wgrad.hip", "wgrad_phased.hip", "norm.hip", "elementwise.hip", "conv0.hip", "posconv.hip", "posconv_direct.hip", "posconv_wgrad.hip",
           "softmax.hip", "attention.hip", "pool.hip", "asp.hip", "tdnn.hip", "wav2spk.hip", "fbank.hip", "augment.hip", "reverb.hip", "skinny.hip", "heads.hip", "margin_head.hip", "score.hip", "score_norm.hip", "backend.hip", "metrics.hip", "calibration.hip", "layer_mix.hip", "ctc.hip", "ctc_long.hip", "optim.hip", "comm.hip"]
HEADERS = ["common.h", "gemm_common.h", "wgrad_common.h", "ctc_common.h", "strip_common.h", "tap_gather.h", "trial_common.h"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]
# per-file additions.  augment.hip: the FIR's 8 outputs x 4 taps are plain v_fmac_f32 at the full f32 vector rate; packed
# into v_pk_fma_f32 pairs (no faster on gfx950) the odd taps need sample pairs at odd offsets, which the compiler
# re-reads from LDS: 20 narrow LDS reads per 16 taps where 8 16-byte reads do (measured at
# 66 rows x 48,000 samples x 2,561 taps: 0.361 ms packed, 0.229 ms plain; profiles/augment_bench.txt)
# calibration.hip: its sums are defined as separate f64 multiplications and additions (include/w2v2_hip.h, "score
# calibration"); the file says so with a pragma, the flag says it to every header it includes as well
EXTRA_FLAGS = {"augment.hip": ["-fno-slp-vectorize"], "calibration.hip": ["-ffp-contract=off"]}


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build libw2v2hip.so")
    return exe


def source_hash() -> str:
    """sha256 over the kernel sources + the C header (what the profiled counters under profiles/ were measured on)."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(SOURCES) + HEADERS:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    h.update(open(os.path.join(HERE, "..", "include", "w2v2_hip.h"), "rb").read())
    return h.hexdigest()[:16]


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.join(HERE, "..", "include", "w2v2_hip.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build_locked(force: bool = False, verbose: bool = False) -> str:
    """build() under an exclusive file lock: concurrent ranks of a data-parallel job build once."""
    import fcntl
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    with open(os.path.join(HERE, "build", ".lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            return build(force=force, verbose=verbose)
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    import time
    t_start = time.time()
    hipcc = _hipcc()
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)

    def compile_one(src: str) -> str:
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        srcp = os.path.join(CSRC, src)
        hdrs = [os.path.join(CSRC, "common.h"), os.path.join(HERE, "..", "include", "w2v2_hip.h")]
        if src.startswith("gemm"):
            hdrs.append(os.path.join(CSRC, "gemm_common.h"))
        if src.startswith("wgrad"):
            hdrs.append(os.path.join(CSRC, "wgrad_common.h"))
        if src.startswith("ctc"):
            hdrs.append(os.path.join(CSRC, "ctc_common.h"))
        if src in ("score.hip", "score_norm.hip", "backend.hip", "metrics.hip"):
            hdrs.append(os.path.join(CSRC, "trial_common.h"))           # (which includes strip_common.h)
        if src in ("tdnn.hip", "wav2spk.hip", "score.hip", "score_norm.hip", "backend.hip", "metrics.hip", "skinny.hip", "conv0.hip"):
            hdrs.append(os.path.join(CSRC, "strip_common.h"))
        if src in ("tdnn.hip", "wav2spk.hip", "conv0.hip"):
            hdrs.append(os.path.join(CSRC, "tap_gather.h"))
        if (not force and os.path.exists(obj)
                and os.path.getmtime(obj) > max(os.path.getmtime(p) for p in [srcp] + hdrs)):
            return obj
        cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-c", srcp, "-o", obj]
        t_obj = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr[-4000:]}")
        os.utime(obj, (t_obj, t_obj))
        if verbose:
            print("compiled", src)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    # the library's timestamp must not run ahead of a source that was edited WHILE the objects were compiling (a later
    # needs_build() would then skip the rebuild): it gets the time at which this build STARTED reading the sources
    tmp = LIB + f".tmp{os.getpid()}"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs + ["-ldl"],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stderr[-4000:]}")
    os.utime(tmp, (t_start, t_start))
    os.replace(tmp, LIB)
    return LIB


if __name__ == "__main__":
    print(build(force=False, verbose=True))
