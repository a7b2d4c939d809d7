"""Thin tensor-level wrappers over the C ABI (include/w2v2_hip.h).

PyTorch is plumbing here: device memory, streams.  Every op enqueues hand-written HIP kernels on the
current torch stream; nothing falls back to torch / CPU arithmetic.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import (BF16, EPI_ADD, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_GRAD, EPI_GELU_BWD, EPI_MUL, EPI_NONE, EPI_SCALE_RC, F16, F32,
                   GemmDesc)

POOL_MODES = {"mean+std": 0, "mean": 1, "max": 2, "first": 3, "first+cls": 3, "last": 4, "middle": 4, "quantile": 5}
POOL_WIDTH = {0: 2, 5: 5}      # output features per input feature (default 1)
POOL_INDEX_BASE = 16           # mode POOL_INDEX_BASE + t selects frame t (IndexPool1D "random")


def lib():
    return _lib.load()


def dt(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float16:
        return F16
    if t.dtype == torch.float32:
        return F32
    raise TypeError(f"unsupported dtype {t.dtype}")


def is16(dtype: torch.dtype) -> bool:
    """A 16-bit activation format (bf16 or IEEE fp16): the matrix-core kernels exist for both."""
    return dtype in (torch.bfloat16, torch.float16)


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("w2v2_speaker_amd ops need tensors on the GPU (no CPU fallback exists)")


class Gemm:
    """A prebuilt GEMM descriptor over fixed buffers: build once, launch every step."""

    def __init__(self, M: int, N: int, K: int, A: torch.Tensor, B: torch.Tensor, Cmat: torch.Tensor, *,
                 lda: int, ldb: int, ldc: int, transA: bool = False, transB: bool = False,
                 batch: int = 1, batch_inner: int = 1,
                 a_strides: Tuple[int, int] = (0, 0), b_strides: Tuple[int, int] = (0, 0),
                 c_strides: Tuple[int, int] = (0, 0),
                 a_seg: Tuple[int, int] = (0, 0), b_seg: Tuple[int, int] = (0, 0),
                 epilogue: int = EPI_NONE, bias: Optional[torch.Tensor] = None, bias_stride1: int = 0,
                 aux: Optional[torch.Tensor] = None, ldaux: int = 0, aux_strides: Tuple[int, int] = (0, 0),
                 row_scale: Optional[torch.Tensor] = None, col_scale: Optional[torch.Tensor] = None,
                 alpha: float = 1.0, split_k: int = 1, accumulate: bool = False,
                 b_lo: Optional[torch.Tensor] = None, n_ext_from: int = 0):
        """b_lo: residual plane of two-term weights (same layout as B, b_lo = T(W - T(W))): output columns
        n >= n_ext_from are computed as A (B + b_lo)^T (include/w2v2_hip.h, w2v2_gemm_desc.k_ext)."""
        _dev(A, B, Cmat, bias, aux, row_scale, col_scale, b_lo)
        if dt(A) != dt(B):
            raise TypeError("GEMM operands must share a dtype")
        if aux is not None and aux.dtype != Cmat.dtype:
            raise TypeError("aux must have the dtype of C")
        for t in (bias, row_scale, col_scale):
            if t is not None and t.dtype != torch.float32:
                raise TypeError("bias / scales are f32")
        d = GemmDesc()
        d.M, d.N, d.K = M, N, K
        d.batch, d.batch_inner = batch, max(1, batch_inner)
        d.dtype_ab, d.dtype_c, d.epilogue = dt(A), dt(Cmat), epilogue
        d.A.ptr, d.A.ld, d.A.trans = A.data_ptr(), lda, int(transA)
        d.A.seg_len, d.A.seg_stride = a_seg
        d.A.stride0, d.A.stride1 = a_strides
        d.B.ptr, d.B.ld, d.B.trans = B.data_ptr(), ldb, int(transB)
        d.B.seg_len, d.B.seg_stride = b_seg
        d.B.stride0, d.B.stride1 = b_strides
        d.C, d.ldc = Cmat.data_ptr(), ldc
        d.c_stride0, d.c_stride1 = c_strides
        d.aux, d.ldaux = _p(aux), ldaux
        d.aux_stride0, d.aux_stride1 = aux_strides
        d.bias, d.bias_stride1 = _p(bias), bias_stride1
        d.row_scale, d.col_scale = _p(row_scale), _p(col_scale)
        d.alpha, d.split_k, d.accumulate = alpha, split_k, int(accumulate)
        d.k_ext, d.n_ext_from, d.b_lo_offset = 0, 0, 0
        if b_lo is not None:
            assert b_lo.dtype == B.dtype and (b_lo.data_ptr() - B.data_ptr()) % B.element_size() == 0
            d.k_ext, d.n_ext_from = K, n_ext_from
            d.b_lo_offset = (b_lo.data_ptr() - B.data_ptr()) // B.element_size()
        self.desc = d
        self._ref = C.byref(d)
        self._keep = (A, B, Cmat, bias, aux, row_scale, col_scale, b_lo)   # keep buffers alive
        self._fn = lib().w2v2_gemm
        self.flops = 2.0 * M * N * K * batch
        # algorithmic HBM bytes: each operand read once, C written once (+ the aux tensor read or written once)
        esz = A.element_size()
        self.bytes = float(batch) * ((M * K + N * K) * esz + M * N * Cmat.element_size() * (2 if aux is not None else 1))
        # which template instantiation of csrc/gemm.hip this descriptor launches (for profiling)
        lp = dt(A) != F32
        self.kernel_class = ("mfma16" if lp else "f32") + "_" + ("t" if transA else "n") + ("n" if transB else "t")
        self.narrow = N <= 64
        self.out_is_act = is16(Cmat.dtype)
        # which kernel this descriptor launches: asked of the library's own dispatch (a dry run of w2v2_gemm, round 5 --
        # the Python mirror of its heuristics could disagree with an env-tuned or differently sized device)
        fam = lib().w2v2_gemm_kernel_of(self._ref)
        self.kernel_name = {4: "gemm16_phased_256x256_kernel", 2: "gemm16_ring_256x128_kernel", 1: "gemm16_dma_128_kernel",
                            3: "gemm16_regstage_kernel", 9: "gemm_f32_mfma_kernel",
                            10: "gemm_f32_dma_kernel"}.get(fam, "gemm16_regstage_kernel" if lp
                                                                                       else "gemm_f32_mfma_kernel")

    _prof = None
    _TIMED_KERNELS = ("gemm16_ring_256x128_kernel", "gemm16_phased_256x256_kernel")
    _log = None        # tools/gemm_instep.py: when a list, every launch appends its shape key (launch order)

    def key(self) -> dict:
        d = self.desc
        return {"kind": "gemm", "M": d.M, "N": d.N, "K": d.K, "batch": d.batch, "epi": d.epilogue,
                "two_term": int(d.k_ext != 0), "n_ext_from": d.n_ext_from, "aux": int(bool(d.aux)),
                "kernel": self.kernel_name, "flops": self.flops + 2.0 * d.M * max(0, d.N - d.n_ext_from) * d.k_ext,
                "alg_flops": self.flops, "bytes": self.bytes}

    @classmethod
    def profile_begin(cls, select) -> None:
        """Time every launch for which select(gemm) is true: by the dispatch's own begin / end timestamps
        (w2v2_gemm_timed: the duration rocprofv3 reports) for the two kernels that have the hook, with a pair of HIP
        events on the launch stream otherwise."""
        cls._prof = {"select": select, "events": [], "slots": []}

    @classmethod
    def profile_end(cls) -> dict:
        prof, cls._prof = cls._prof, None
        if not prof or not (prof["events"] or prof["slots"]):
            return {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "by_kernel": {}}
        torch.cuda.synchronize()
        out = {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "by_kernel": {}}
        timed = []
        if prof["slots"]:
            import ctypes
            buf = (ctypes.c_float * len(prof["slots"]))()
            _lib.check(lib().w2v2_timer_read(0, len(prof["slots"]), ctypes.cast(buf, ctypes.c_void_p)), "timer_read")
            timed = [(float(buf[i]),) + prof["slots"][i] for i in range(len(prof["slots"]))]
        for ms, f, nb, name in [(a.elapsed_time(b), f, nb, name) for a, b, f, nb, name in prof["events"]] + timed:
            k = out["by_kernel"].setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            for d in (out, k):
                d["launches"] += 1
                d["ms"] += ms
                d["flops"] += f
                d["bytes"] += nb
        return out

    def __call__(self) -> None:
        prof = Gemm._prof
        if Gemm._log is not None:
            Gemm._log.append(self.key())
        if (prof is not None and prof["select"](self) and self.kernel_name in Gemm._TIMED_KERNELS
                and hasattr(lib(), "w2v2_gemm_timed")):
            rc = lib().w2v2_gemm_timed(self._ref, stream(), len(prof["slots"]))
            prof["slots"].append((self.flops, self.bytes, self.kernel_name))
        elif prof is not None and prof["select"](self):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = self._fn(self._ref, stream())
            e1.record()
            prof["events"].append((e0, e1, self.flops, self.bytes, self.kernel_name))
        else:
            rc = self._fn(self._ref, stream())
        if rc:
            _lib.check(rc, "gemm")


def gemm(*args, **kw) -> None:
    Gemm(*args, **kw)()


class WgradGroup:
    """Prebuilt grouped weight-gradient launch: problems = [(dY, X, dW, dbias or None), ...] with
    dY [Tpad, n_out] / X [Tpad, n_in] bf16 (rows >= tokens zero) and dW [n_out, n_in] f32."""

    def __init__(self, problems, tokens: int, tokens_padded: int):
        n = len(problems)
        arr = (_lib.WgradProblem * n)()
        keep = []
        self.flops = 0.0
        for i, (dY, X, dW, db) in enumerate(problems):
            _dev(dY, X, dW, db)
            assert is16(dY.dtype) and X.dtype == dY.dtype and dW.dtype == torch.float32
            assert i == 0 or dY.dtype == problems[0][0].dtype, "one element type per grouped launch"
            assert dY.shape[0] >= tokens_padded and X.shape[0] >= tokens_padded
            q = arr[i]
            q.dY, q.ld_dy = dY.data_ptr(), dY.stride(0)
            q.X, q.ld_x = X.data_ptr(), X.stride(0)
            q.dW, q.ld_dw = dW.data_ptr(), dW.stride(0)
            q.dbias = _p(db)
            q.n_out, q.n_in = dW.shape
            keep.append((dY, X, dW, db))
            self.flops += 2.0 * tokens * dW.shape[0] * dW.shape[1]
        self._arr, self._keep, self._n = arr, keep, n
        self._tokens, self._tpad = tokens, tokens_padded
        self._dt = dt(problems[0][0])
        self._fn = lib().w2v2_wgrad_grouped
        # which kernel this group launches (for the in-step profile labels): asked of the library's own routing, like
        # Gemm.kernel_name (csrc/wgrad.hip wgrad_route: switches, forced family and the device's CU count included)
        self.kernel_name = self._KERNELS.get(lib().w2v2_wgrad_kernel_of(arr, n), "rejected")   # (> 32 problems: the launch raises)

    _KERNELS = {1: "wgrad_grouped_kernel", 2: "wgrad_grouped_ring_kernel", 3: "wgrad_grouped_ring4_kernel",
                4: "wgrad_grouped_phased_kernel"}

    def __call__(self) -> None:
        if Gemm._log is not None:
            Gemm._log.append({"kind": "wgrad", "problems": self._n, "tokens": self._tokens, "flops": self.flops,
                              "alg_flops": self.flops,
                              "kernel": self.kernel_name})
        rc = self._fn(self._arr, self._n, self._tokens, self._tpad, self._dt, stream())
        if rc:
            _lib.check(rc, "wgrad_grouped")


# ------------------------------------------------------------------------------------------------ conv0
def conv0_workspace(B: int, N: int, C: int, k: int, stride: int, device) -> torch.Tensor:
    """f32 scratch for conv0_groupnorm_gelu: per-chunk partial sums + {mean, rstd}."""
    n = lib().w2v2_conv0_workspace_floats(N, C, k, stride)
    return torch.empty(B * n + B * C * 2, dtype=torch.float32, device=device)


def conv0_groupnorm_gelu(wav: torch.Tensor, w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                         out: torch.Tensor, work: torch.Tensor, k: int, stride: int, eps: float = 1e-5) -> None:
    """HF:302-323 layer 0.  wav [B,N] f32, w [C,1,k] f32, out [B,L,C], work from conv0_workspace()."""
    _dev(wav, w, gamma, beta, out, work)
    B, N = wav.shape
    Cc = w.shape[0]
    mr = work[work.numel() - B * Cc * 2:]
    L = lib()
    # 16-bit activations: conv on the matrix cores (split-bf16, ~2^-16); statistics from the waveform's window moments
    stats = L.w2v2_conv0_stats_mfma if is16(out.dtype) else L.w2v2_conv0_stats
    _lib.check(stats(wav.data_ptr(), w.data_ptr(), work.data_ptr(), mr.data_ptr(), B, N, Cc, k, stride,
                     eps, stream()), "conv0_stats")
    _lib.check(L.w2v2_conv0_apply(wav.data_ptr(), w.data_ptr(), mr.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                  out.data_ptr(), dt(out), B, N, Cc, k, stride, stream()), "conv0_apply")


def conv0_stats_len(wav, w, work, frames, k: int, stride: int, mfma: bool, eps: float = 1e-5) -> torch.Tensor:
    """Variable-length conv-0 GroupNorm statistics: frames = device int32 [B] valid frames per utterance.  Returns the
    {mean, rstd} view [B, C, 2] of `work` (conv0_workspace())."""
    _dev(wav, w, work, frames)
    assert frames.dtype == torch.int32
    B, N = wav.shape
    Cc = w.shape[0]
    mr = work[work.numel() - B * Cc * 2:]
    fn = lib().w2v2_conv0_stats_mfma_len if mfma else lib().w2v2_conv0_stats_len
    _lib.check(fn(wav.data_ptr(), w.data_ptr(), work.data_ptr(), mr.data_ptr(), frames.data_ptr(), B, N, Cc, k, stride,
                  eps, stream()), "conv0_stats_len")
    return mr.view(B, Cc, 2)


def conv0_groupnorm_gelu_len(wav, w, gamma, beta, out, work, frames, k: int, stride: int, eps: float = 1e-5) -> None:
    """conv0_groupnorm_gelu with the GroupNorm statistics of each utterance over its first frames[b] frames (the apply
    pass is per frame and needs no lengths; frames past the end are computed and left unspecified)."""
    _dev(wav, w, gamma, beta, out, work, frames)
    B, N = wav.shape
    Cc = w.shape[0]
    mr = conv0_stats_len(wav, w, work, frames, k, stride, is16(out.dtype), eps)
    _lib.check(lib().w2v2_conv0_apply(wav.data_ptr(), w.data_ptr(), mr.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                      out.data_ptr(), dt(out), B, N, Cc, k, stride, stream()), "conv0_apply")


def conv0_layernorm_gelu(wav, w, bias, gamma, beta, out, k: int, stride: int, eps: float = 1e-5) -> None:
    """Layer 0 of the feat_extract_norm="layer" family: out [B, L, C] = GELU(LN_C(conv0(wav) + bias)) (HF:275-299)."""
    _dev(wav, w, bias, gamma, beta, out)
    B, N = wav.shape
    _lib.check(lib().w2v2_conv0_layernorm_gelu(wav.data_ptr(), w.data_ptr(), _p(bias), gamma.data_ptr(), beta.data_ptr(),
                                               out.data_ptr(), B, N, out.shape[-1], k, stride, eps, dt(out), stream()),
               "conv0_layernorm_gelu")


def conv0_layernorm_gelu_bwd_workspace(B: int, N: int, C: int, k: int, stride: int, device) -> torch.Tensor:
    """f32 scratch of conv0_layernorm_gelu_bwd: one partial row [k + 3][C] per workgroup."""
    n = lib().w2v2_conv0_layernorm_gelu_bwd_workspace_floats(B, N, C, k, stride)
    return torch.empty(max(n, 1), dtype=torch.float32, device=device)


def conv0_layernorm_gelu_bwd(wav, w, bias, gamma, beta, dy, dw, dbias, dgamma, dbeta, work, k: int, stride: int,
                             eps: float = 1e-5) -> None:
    """Backward of conv0_layernorm_gelu: dy [B, L, C] -> dw [C, 1, k], dbias (None with bias None), dgamma, dbeta, all
    ADDED (fixed-order sums: bitwise reproducible); `work` from conv0_layernorm_gelu_bwd_workspace()."""
    _dev(wav, w, bias, gamma, beta, dy, dw, dbias, dgamma, dbeta, work)
    B, N = wav.shape
    Cc = dy.shape[-1]
    if work.numel() < lib().w2v2_conv0_layernorm_gelu_bwd_workspace_floats(B, N, Cc, k, stride):
        raise ValueError("conv0_layernorm_gelu_bwd: workspace too small")
    _lib.check(lib().w2v2_conv0_layernorm_gelu_bwd(wav.data_ptr(), w.data_ptr(), _p(bias), gamma.data_ptr(), beta.data_ptr(),
                                                   dy.data_ptr(), dw.data_ptr(), _p(dbias), dgamma.data_ptr(),
                                                   dbeta.data_ptr(), work.data_ptr(), B, N, Cc, k, stride, eps, dt(dy),
                                                   stream()), "conv0_layernorm_gelu_bwd")


def conv0_bwd(wav, w, work, gamma, beta, dz, sums, dw, dgamma, dbeta, k: int, stride: int) -> None:
    """Backward of layer 0 (see w2v2_conv0_bwd); `work` is the forward's conv0 workspace (holds mean/rstd)."""
    _dev(wav, w, work, gamma, beta, dz, sums, dw, dgamma, dbeta)
    B, N = wav.shape
    Cc = w.shape[0]
    mr = work[work.numel() - B * Cc * 2:]
    _lib.check(lib().w2v2_conv0_bwd(wav.data_ptr(), w.data_ptr(), mr.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                    dz.data_ptr(), sums.data_ptr(), dw.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                    dt(dz), B, N, Cc, k, stride, stream()), "conv0_bwd")


def col2im(col, dx, B: int, Lin: int, Lout: int, Cin: int, k: int, stride: int) -> None:
    _dev(col, dx)
    _lib.check(lib().w2v2_col2im(col.data_ptr(), dx.data_ptr(), B, Lin, Lout, Cin, k, stride, dt(col), stream()),
               "col2im")


def unpack_conv_grad(gp, g) -> None:
    _dev(gp, g)
    co, ci, k = g.shape
    _lib.check(lib().w2v2_unpack_conv_grad(gp.data_ptr(), g.data_ptr(), co, ci, k, stream()), "unpack_conv_grad")


def pack_conv_weight(w: torch.Tensor, out: torch.Tensor) -> None:
    _dev(w, out)
    co, ci, k = w.shape
    _lib.check(lib().w2v2_pack_conv_weight(w.data_ptr(), out.data_ptr(), dt(out), co, ci, k, stream()), "pack_conv")


# ------------------------------------------------------------------------------------------------ norm
def layernorm_fwd(x, r, gamma, beta, y, mean, rstd, eps: float, drop_p: float = 0.0, seed: int = 0) -> None:
    _dev(x, r, gamma, beta, y, mean, rstd)
    H = x.shape[-1]
    M = x.numel() // H
    _lib.check(lib().w2v2_layernorm_fwd(x.data_ptr(), _p(r), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                        mean.data_ptr(), rstd.data_ptr(), M, H, eps, drop_p, seed, dt(x), stream()),
               "layernorm_fwd")


def layernorm_gelu_fwd(x, gamma, beta, y, eps: float) -> None:
    """y = GELU(LN(x)): the convolution layers of the feat_extract_norm="layer" family (HF:275-299)."""
    _dev(x, gamma, beta, y)
    H = x.shape[-1]
    _lib.check(lib().w2v2_layernorm_gelu_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), x.numel() // H, H,
                                             eps, dt(x), stream()), "layernorm_gelu_fwd")


def layernorm_gelu_bwd_workspace(M: int, H: int, device) -> torch.Tensor:
    """f32 scratch of layernorm_gelu_bwd: one partial row [3][H] per workgroup."""
    return torch.empty(max(lib().w2v2_layernorm_gelu_bwd_workspace_floats(M, H), 1), dtype=torch.float32, device=device)


def layernorm_gelu_bwd(dy, z, gamma, beta, dz, dgamma, dbeta, dbias, work, eps: float = 1e-5) -> None:
    """Backward of layernorm_gelu_fwd from the saved pre-norm z: dz (may alias dy) written, dgamma / dbeta / dbias (the
    column sum of dz, may be None) ADDED in a fixed order (bitwise reproducible); `work` from layernorm_gelu_bwd_workspace()."""
    _dev(dy, z, gamma, beta, dz, dgamma, dbeta, dbias, work)
    H = dy.shape[-1]
    M = dy.numel() // H
    if work.numel() < lib().w2v2_layernorm_gelu_bwd_workspace_floats(M, H):
        raise ValueError("layernorm_gelu_bwd: workspace too small")
    _lib.check(lib().w2v2_layernorm_gelu_bwd(dy.data_ptr(), z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dz.data_ptr(),
                                             dgamma.data_ptr(), dbeta.data_ptr(), _p(dbias), work.data_ptr(), M, H, eps,
                                             dt(dy), stream()), "layernorm_gelu_bwd")


_LN_WS = {}


def _ln_workspace(H: int, device) -> torch.Tensor:
    key = (H, str(device))
    if key not in _LN_WS:
        _LN_WS[key] = torch.empty(lib().w2v2_layernorm_bwd_workspace_floats(H), dtype=torch.float32, device=device)
    return _LN_WS[key]


def layernorm_bwd(dy, s, mean, rstd, gamma, ds, d_r, dgamma, dbeta, drop_p: float = 0.0, seed: int = 0,
                  defer_to: Optional["LnFoldGroup"] = None) -> None:
    """With ``defer_to`` the column partials stay in a workspace of that group and dgamma/dbeta are folded later by
    ``defer_to.fold()`` (one launch for up to 8 LayerNorms)."""
    _dev(dy, s, mean, rstd, gamma, ds, d_r, dgamma, dbeta)
    H = dy.shape[-1]
    M = dy.numel() // H
    if defer_to is not None and dgamma is not None:
        ws = defer_to.add(dgamma, dbeta, M, H)
        _lib.check(lib().w2v2_layernorm_bwd(dy.data_ptr(), s.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                            gamma.data_ptr(), ds.data_ptr(), _p(d_r), None, None, ws.data_ptr(), M, H,
                                            drop_p, seed, dt(dy), stream()), "layernorm_bwd")
        return
    ws = _ln_workspace(H, dy.device) if dgamma is not None else None
    _lib.check(lib().w2v2_layernorm_bwd(dy.data_ptr(), s.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                        gamma.data_ptr(), ds.data_ptr(), _p(d_r), _p(dgamma), _p(dbeta), _p(ws), M, H,
                                        drop_p, seed, dt(dy), stream()), "layernorm_bwd")


class LnFoldGroup:
    """Pending LayerNorm gamma/beta folds of one gradient bucket: each deferred layernorm_bwd gets its own workspace
    slot (allocated once), fold() issues ONE w2v2_layernorm_bwd_fold launch for all of them."""

    def __init__(self, H: int, device, slots: int = 8):
        n = lib().w2v2_layernorm_bwd_workspace_floats(H)
        self._ws = torch.empty(slots, n, dtype=torch.float32, device=device)
        self._arr = (_lib.LnFold * slots)()
        self._n, self._M, self._H, self._keep = 0, 0, H, []

    def add(self, dgamma, dbeta, M: int, H: int) -> torch.Tensor:
        if self._n == len(self._arr):
            self.fold()
        assert H == self._H and (self._n == 0 or M == self._M)
        e = self._arr[self._n]
        e.partial, e.dgamma, e.dbeta = self._ws[self._n].data_ptr(), dgamma.data_ptr(), dbeta.data_ptr()
        self._keep.append((dgamma, dbeta))
        self._M = M
        self._n += 1
        return self._ws[self._n - 1]

    def fold(self) -> None:
        if self._n:
            _lib.check(lib().w2v2_layernorm_bwd_fold(self._arr, self._n, self._M, self._H, stream()),
                       "layernorm_bwd_fold")
        self._n, self._keep = 0, []


# ------------------------------------------------------------------------------------------------ elementwise
def dropout_(x: torch.Tensor, p: float, seed: int) -> None:
    _dev(x)
    _lib.check(lib().w2v2_dropout(x.data_ptr(), x.data_ptr(), x.numel(), p, seed, dt(x), stream()), "dropout")


def dropout(x: torch.Tensor, y: torch.Tensor, p: float, seed: int) -> None:
    """y = dropout(x): the kernel and keep-mask of ``dropout_``, written to another tensor of the same type and size."""
    _dev(x, y)
    assert x.dtype == y.dtype and x.numel() == y.numel() and x.is_contiguous() and y.is_contiguous()
    _lib.check(lib().w2v2_dropout(x.data_ptr(), y.data_ptr(), x.numel(), p, seed, dt(x), stream()), "dropout")


def gelu_bwd(dy, pre, dx) -> None:
    _dev(dy, pre, dx)
    _lib.check(lib().w2v2_gelu_bwd(dy.data_ptr(), pre.data_ptr(), dx.data_ptr(), dy.numel(), dt(dy), stream()),
               "gelu_bwd")


PARTIAL_ROWS = 256              # W2V2_PARTIAL_ROWS (include/w2v2_hip.h): rows of a fixed-order column-sum workspace
_PARTIAL_WS = {}


def _partial_workspace(N: int, device, st: int) -> torch.Tensor:
    """[PARTIAL_ROWS, N] f32 partial column sums of gelu_bwd_colsum / mask_fill_bwd: one per (N, device, stream st).  Calls
    on one stream share it safely (the fold that reads it is enqueued before the next call can write it); a call on
    another stream gets a workspace of its own, so two streams never race on one."""
    key = (N, str(device), st)
    if key not in _PARTIAL_WS:
        _PARTIAL_WS[key] = torch.empty(PARTIAL_ROWS * N, dtype=torch.float32, device=device)
    return _PARTIAL_WS[key]


def gelu_bwd_colsum(dy, pre, dx, colsum_out, M: int, N: int) -> None:
    """dx = dy * gelu'(pre) over [M, N] and colsum_out[n] += sum_m dx[m, n] (fixed order: bitwise reproducible)."""
    _dev(dy, pre, dx, colsum_out)
    st = stream()
    ws = _partial_workspace(N, dy.device, st)
    _lib.check(lib().w2v2_gelu_bwd_colsum(dy.data_ptr(), pre.data_ptr(), dx.data_ptr(), colsum_out.data_ptr(),
                                          ws.data_ptr(), M, N, dt(dy), st), "gelu_bwd_colsum")


def add(x, a, y) -> None:
    _dev(x, a, y)
    _lib.check(lib().w2v2_add(x.data_ptr(), a.data_ptr(), y.data_ptr(), x.numel(), dt(x), stream()), "add")


def colsum(x: torch.Tensor, out: torch.Tensor, M: int, N: int, ld: Optional[int] = None) -> None:
    """out[n] += sum_m x[m][n] (f32 atomics)."""
    _dev(x, out)
    _lib.check(lib().w2v2_colsum(x.data_ptr(), ld if ld is not None else N, out.data_ptr(), M, N, dt(x), stream()),
               "colsum")


def zero_ranges(base: torch.Tensor, table: torch.Tensor, blocks_per_range: int = 8) -> None:
    """base[off : off + n] = 0 for every (off, n) row of the int64 device table (f32 arena)."""
    _dev(base, table)
    assert base.dtype == torch.float32 and table.dtype == torch.int64
    _lib.check(lib().w2v2_zero_ranges(base.data_ptr(), table.data_ptr(), table.shape[0], blocks_per_range, stream()),
               "zero_ranges")


def mean(x: torch.Tensor, out: torch.Tensor) -> None:
    _dev(x, out)
    assert x.dtype == torch.float32 and out.dtype == torch.float32
    _lib.check(lib().w2v2_mean(x.data_ptr(), out.data_ptr(), x.numel(), stream()), "mean")


def cast(x: torch.Tensor, y: torch.Tensor) -> None:
    _dev(x, y)
    _lib.check(lib().w2v2_cast(x.data_ptr(), y.data_ptr(), x.numel(), dt(y), stream()), "cast")


def transpose_many(src, dst, table, n: int, blocks_per_matrix: int = 64) -> None:
    _dev(src, dst, table)
    _lib.check(lib().w2v2_transpose_many(src.data_ptr(), dst.data_ptr(), table.data_ptr(), n, blocks_per_matrix,
                                         dt(src), stream()), "transpose_many")


def mask_fill(h, mask_u8, embed) -> None:
    _dev(h, mask_u8, embed)
    H = h.shape[-1]
    _lib.check(lib().w2v2_mask_fill(h.data_ptr(), mask_u8.data_ptr(), embed.data_ptr(), h.numel() // H, H, dt(h),
                                    stream()), "mask_fill")


def mask_feature(h, mask_u8, B: int, T: int) -> None:
    """h [B*T, H] (or [B, T, H]): channels c with mask_u8[b][c] != 0 are zeroed for every frame of utterance b."""
    _dev(h, mask_u8)
    H = h.shape[-1]
    assert mask_u8.dtype == torch.uint8 and mask_u8.numel() == B * H
    _lib.check(lib().w2v2_mask_feature(h.data_ptr(), mask_u8.data_ptr(), B, T, H, dt(h), stream()), "mask_feature")


def mask_fill_bwd(dh, mask_u8, d_embed) -> None:
    _dev(dh, mask_u8, d_embed)
    H = dh.shape[-1]
    st = stream()
    ws = _partial_workspace(H, dh.device, st)
    _lib.check(lib().w2v2_mask_fill_bwd(dh.data_ptr(), mask_u8.data_ptr(), d_embed.data_ptr(), ws.data_ptr(),
                                        dh.numel() // H, H, dt(dh), st), "mask_fill_bwd")


def prepend_token(x, y, c: float) -> None:
    _dev(x, y)
    B, T, H = x.shape
    _lib.check(lib().w2v2_prepend_token(x.data_ptr(), y.data_ptr(), c, B, T, H, dt(x), stream()), "prepend_token")


def pair_tables(left_row, left_frames, right_row, right_frames, rows: int, T: int) -> torch.Tensor:
    """The four tables of pair_assemble as one CPU int32 tensor [4, B], checked against a feature matrix of ``rows`` rows
    and sequences of ``T`` frames (the kernel trusts them): both sides at least one frame, [CLS] left [SEP] right [SEP]
    within T, both row ranges inside the matrix.  Host only."""
    as_list = lambda x: x.reshape(-1).tolist() if isinstance(x, torch.Tensor) else list(x)
    cols = [[int(v) for v in as_list(x)] for x in (left_row, left_frames, right_row, right_frames)]
    if len({len(c) for c in cols}) != 1 or not cols[0]:
        raise ValueError("pair_assemble: the four tables need one entry per pair (at least one pair)")
    for b, (lr, ta, rr, tb) in enumerate(zip(*cols)):
        if ta < 1 or tb < 1:
            raise ValueError(f"pair_assemble: pair {b} has an empty side ({ta} + {tb} frames)")
        if ta + tb + 3 > T:
            raise ValueError(f"pair_assemble: pair {b} needs {ta + tb + 3} frames, the sequence has {T}")
        if lr < 0 or rr < 0 or lr + ta > rows or rr + tb > rows:
            raise ValueError(f"pair_assemble: pair {b} reads rows [{lr}, {lr + ta}) and [{rr}, {rr + tb}) of a feature "
                             f"matrix of {rows}")
    return torch.tensor(cols, dtype=torch.int32)


def pair_assemble(feat, y, left_row, left_frames, right_row, right_frames, cls_c: float, sep_c: float,
                  table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [B, T, H] = [CLS] left [SEP] right [SEP] 0... per pair from rows of feat [R, H] (w2v2_pair_assemble).  The tables
    are host values (Python ints or CPU integer tensors): validated here (ValueError), then uploaded into ``table``
    (device int32 [4, B]; allocated when None).  Returns the checked host tables (CPU int32 [4, B])."""
    _dev(feat, y)
    B, T, H = y.shape
    assert feat.dim() == 2 and feat.shape[1] == H and feat.dtype == y.dtype and feat.is_contiguous() and y.is_contiguous()
    host = pair_tables(left_row, left_frames, right_row, right_frames, feat.shape[0], T)
    if host.shape[1] != B:
        raise ValueError(f"pair_assemble: {host.shape[1]} pairs for a batch of {B}")
    if table is None:
        table = torch.empty(4, B, dtype=torch.int32, device=y.device)
    assert table.shape == (4, B) and table.dtype == torch.int32 and table.is_cuda and table.is_contiguous()
    table.copy_(host)
    _lib.check(lib().w2v2_pair_assemble(feat.data_ptr(), y.data_ptr(), table[0].data_ptr(), table[1].data_ptr(),
                                        table[2].data_ptr(), table[3].data_ptr(), cls_c, sep_c, B, T, H, dt(y), stream()),
               "pair_assemble")
    return host


# ------------------------------------------------------------------------------------------------ pos-conv
def posconv_wgrad(dY, xg, dwf, B: int, T: int, H: int, G: int, K: int) -> None:
    """dwf[g][(tap, ci)][co] = sum_{b,t} xg[b,g,t+tap,ci] * dY[b,t,g*Cg+co]  (bf16 operands, f32 result, overwritten)."""
    _dev(dY, xg, dwf)
    assert is16(dY.dtype) and xg.dtype == dY.dtype and dwf.dtype == torch.float32
    _lib.check(lib().w2v2_posconv_wgrad(dY.data_ptr(), xg.data_ptr(), dwf.data_ptr(), B, T, H, G, K, dt(dY), stream()),
               "posconv_wgrad")


def posconv_direct(xg, w, out, aux, bias, B: int, T: int, G: int, Cg: int, K: int, ldc: int, mode: int) -> None:
    """Direct grouped pos-conv / its data gradient (include/w2v2_hip.h w2v2_posconv_direct): mode 0 = GELU(conv + bias)
    (+ pre-activation into aux), mode 1 = conv + aux."""
    _dev(xg, w, out, aux, bias)
    assert is16(xg.dtype) and w.dtype == xg.dtype and out.dtype == xg.dtype
    _lib.check(lib().w2v2_posconv_direct(xg.data_ptr(), w.data_ptr(), out.data_ptr(), _p(aux), _p(bias), B, T, G, Cg, K,
                                         ldc, mode, dt(xg), stream()), "posconv_direct")
    if Gemm._log is not None:
        Gemm._log.append({"kind": "posconv", "flops": 2.0 * B * T * G * Cg * K * Cg, "alg_flops": 2.0 * B * T * G * Cg * K * Cg,
                          "kernel": "posconv_direct_kernel", "M": B * T, "N": Cg, "K": K * Cg, "mode": mode})


def posconv_regroup(x, xg, B: int, T: int, H: int, G: int, K: int, pad_left: int) -> None:
    _dev(x, xg)
    _lib.check(lib().w2v2_posconv_regroup(x.data_ptr(), xg.data_ptr(), B, T, H, G, K, pad_left, dt(x), stream()),
               "posconv_regroup")


def posconv_regroup_len(x, xg, lens, B: int, T: int, H: int, G: int, K: int, pad_left: int) -> None:
    """posconv_regroup with frames t >= lens[b] (device int32 [B]) written as zeros."""
    _dev(x, xg, lens)
    _lib.check(lib().w2v2_posconv_regroup_len(x.data_ptr(), xg.data_ptr(), lens.data_ptr(), B, T, H, G, K, pad_left,
                                              dt(x), stream()), "posconv_regroup_len")


def weightnorm_scratch(H: int, G: int, K: int, device) -> torch.Tensor:
    """f32 scratch of weightnorm_pack (``sumsq``) / weightnorm_bwd (``dot``): per-tap result + per-block partials."""
    return torch.empty(int(lib().w2v2_weightnorm_scratch_floats(H, G, K)), dtype=torch.float32, device=device)


def weightnorm_pack(g, v, sumsq, wf, wb, H: int, G: int, K: int) -> None:
    _dev(g, v, sumsq, wf, wb)
    _lib.check(lib().w2v2_weightnorm_pack(g.data_ptr(), v.data_ptr(), sumsq.data_ptr(), wf.data_ptr(),
                                          wb.data_ptr(), H, G, K, dt(wf), stream()), "weightnorm_pack")


def weightnorm_bwd(g, v, sumsq, dwf, dot, dg, dv, H: int, G: int, K: int) -> None:
    _dev(g, v, sumsq, dwf, dot, dg, dv)
    _lib.check(lib().w2v2_weightnorm_bwd(g.data_ptr(), v.data_ptr(), sumsq.data_ptr(), dwf.data_ptr(),
                                         dot.data_ptr(), dg.data_ptr(), dv.data_ptr(), H, G, K, stream()),
               "weightnorm_bwd")


# ------------------------------------------------------------------------------------------------ attention
def softmax_fwd(s, p, p_drop, rows: int, T: int, ld: int, drop_p: float, seed: int) -> None:
    _dev(s, p, p_drop)
    _lib.check(lib().w2v2_softmax_fwd(s.data_ptr(), p.data_ptr(), _p(p_drop), rows, T, ld, drop_p, seed, dt(p),
                                      stream()), "softmax_fwd")


def softmax_fwd_len(s, p, lens, B: int, heads: int, T: int, ld: int) -> None:
    """Eval softmax of a variable-length batch: rows B * heads * T, keys < lens[b] (device int32 [B]), padded rows zero."""
    _dev(s, p, lens)
    _lib.check(lib().w2v2_softmax_fwd_len(s.data_ptr(), p.data_ptr(), lens.data_ptr(), B, heads, T, ld, dt(p),
                                          stream()), "softmax_fwd_len")


def softmax_bwd(dp_drop, p, ds, rows: int, T: int, ld: int, drop_p: float, seed: int) -> None:
    _dev(dp_drop, p, ds)
    _lib.check(lib().w2v2_softmax_bwd(dp_drop.data_ptr(), p.data_ptr(), ds.data_ptr(), rows, T, ld, drop_p, seed,
                                      dt(p), stream()), "softmax_bwd")


def attention_fwd(qkv, ctx, lse, B: int, T: int, heads: int, d: int, scale: float, drop_p: float, seed: int) -> None:
    _dev(qkv, ctx, lse)
    _lib.check(lib().w2v2_attention_fwd(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), B, T, heads, d, scale,
                                        drop_p, seed, dt(qkv), stream()), "attention_fwd")


def attention_fwd_len(qkv, ctx, lse, lens, B: int, T: int, heads: int, d: int, scale: float) -> None:
    """Eval fused attention of a variable-length batch: utterance b attends over its first lens[b] (device int32 [B])
    frames; ctx rows past them are zeros."""
    _dev(qkv, ctx, lse, lens)
    _lib.check(lib().w2v2_attention_fwd_len(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), lens.data_ptr(), B, T, heads,
                                            d, scale, dt(qkv), stream()), "attention_fwd_len")


def attention_bwd(qkv, ctx, dctx, lse, dqkv, delta, B: int, T: int, heads: int, d: int, scale: float,
                  drop_p: float, seed: int) -> None:
    _dev(qkv, ctx, dctx, lse, dqkv, delta)
    _lib.check(lib().w2v2_attention_bwd(qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(),
                                        dqkv.data_ptr(), delta.data_ptr(), B, T, heads, d, scale, drop_p, seed,
                                        dt(qkv), stream()), "attention_bwd")


# ------------------------------------------------------------------------------------------------ pooling
def pool_fwd(x, out, mode: int) -> None:
    _dev(x, out)
    B, T, H = x.shape
    _lib.check(lib().w2v2_pool_fwd(x.data_ptr(), out.data_ptr(), B, T, H, mode, dt(x), stream()), "pool_fwd")


def pool_fwd_len(x, out, lens, mode: int) -> None:
    """pool_fwd over the first lens[b] (device int32 [B]) frames of each utterance of x [B, T, H]."""
    _dev(x, out, lens)
    B, T, H = x.shape
    _lib.check(lib().w2v2_pool_fwd_len(x.data_ptr(), out.data_ptr(), lens.data_ptr(), B, T, H, mode, dt(x), stream()),
               "pool_fwd_len")


def pool_bwd(x, out, dout, dx, mode: int) -> None:
    _dev(x, out, dout, dx)
    B, T, H = x.shape
    _lib.check(lib().w2v2_pool_bwd(x.data_ptr(), out.data_ptr(), dout.data_ptr(), dx.data_ptr(), B, T, H, mode,
                                   dt(x), stream()), "pool_bwd")


# ------------------------------------------------------------------------------------------------ layer mix
LAYER_MIX_MAX_STATES = 32      # W2V2_LAYER_MIX_MAX_STATES
LAYER_MIX_LDS_FRAMES = 512     # W2V2_LAYER_MIX_LDS_FRAMES: longer inputs stage m in a caller-owned f32 buffer
_MIX_X = (torch.float32, torch.bfloat16, torch.float16)
_MIX_Y = (torch.float32, torch.bfloat16)


def _is_f32_vec(t, n: int) -> bool:
    return isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == n and t.is_contiguous()


class LayerMixTable:
    """The device table of J base pointers the layer-mix kernels read their hidden states through (include/w2v2_hip.h,
    "layer mix"): J tensors of one shape [..., H] and dtype, each contiguous -- built once per plan."""

    def __init__(self, states):
        states = list(states)
        if not 1 <= len(states) <= LAYER_MIX_MAX_STATES:
            raise ValueError(f"layer_mix_table: 1 .. {LAYER_MIX_MAX_STATES} hidden states, got {len(states)}")
        x0 = states[0]
        for x in states:
            if not isinstance(x, torch.Tensor) or x.dtype not in _MIX_X or x.dim() < 2:
                raise ValueError("layer_mix_table: hidden states are f32, bf16 or f16 tensors [..., H]")
            if x.shape != x0.shape or x.dtype != x0.dtype or not x.is_contiguous():
                raise ValueError("layer_mix_table: hidden states must share one shape and dtype and be contiguous")
        self.H, self.rows, self.J, self.dtype = int(x0.shape[-1]), x0.numel() // int(x0.shape[-1]), len(states), x0.dtype
        if self.H % 8 or self.H < 8:
            raise ValueError(f"layer_mix_table: H must be a multiple of 8 (16-byte vector accesses), got {self.H}")
        if any(x.data_ptr() % 16 for x in states):
            raise ValueError("layer_mix_table: hidden states need 16-byte aligned bases")
        _dev(*states)
        self.ptrs = torch.tensor([x.data_ptr() for x in states], dtype=torch.int64).to(x0.device)
        self._keep = states


def _mix_check(name: str, table, logits, B: int, T: int, y, ldy: int, rstd, instance_norm: bool) -> None:
    if not isinstance(table, LayerMixTable):
        raise ValueError(f"{name}: table is a LayerMixTable")
    if B < 1 or T < 1 or B * T != table.rows:
        raise ValueError(f"{name}: B x T = {B} x {T} does not match the table's {table.rows} rows")
    if not _is_f32_vec(logits, table.J):
        raise ValueError(f"{name}: logits is a contiguous float32 vector of {table.J} values")
    if not isinstance(y, torch.Tensor) or y.dtype not in _MIX_Y:
        raise ValueError(f"{name}: y is a float32 or bfloat16 tensor")
    if ldy < table.H or ldy % 8 or y.numel() < (B * T - 1) * ldy + table.H or y.data_ptr() % 16:
        raise ValueError(f"{name}: y needs a 16-byte aligned base, a row stride >= H = {table.H} that is a multiple of 8 "
                         f"and B * T rows (stride {ldy}, {y.numel()} elements)")
    if instance_norm and not _is_f32_vec(rstd.reshape(-1) if isinstance(rstd, torch.Tensor) else rstd, B * table.H):
        raise ValueError(f"{name}: instance_norm needs rstd, contiguous float32 [B, H]")


def layer_mix_workspace(B: int, T: int, H: int, J: int, device) -> torch.Tensor:
    """The f32 workspace of layer_mix_bwd: one row of per-workgroup partials of the J logit gradients per workgroup."""
    n = lib().w2v2_layer_mix_workspace_floats(B, T, H, J)
    if n < 0:
        raise ValueError(f"layer_mix_workspace: bad shape B {B}, T {T}, H {H} (a multiple of 8), J {J} (1 .. {LAYER_MIX_MAX_STATES})")
    return torch.empty(n, dtype=torch.float32, device=device)


def layer_mix_fwd(table: LayerMixTable, logits, y, ldy: int, B: int, T: int, rstd=None, lens=None, w_out=None, stage=None,
                  instance_norm: bool = True) -> None:
    """y[b,t,:H] = instance norm over time of sum_j softmax(logits)_j x_j (include/w2v2_hip.h, "layer mix"); y is the
    ECAPA plan's feature buffer (f32 / bf16, row stride ldy).  lens: device int32 [B] frame counts or None.  w_out: f32
    [J] receives the softmax weights.  stage: f32 [B * T, H], needed beyond LAYER_MIX_LDS_FRAMES frames."""
    name = "layer_mix_fwd"
    _mix_check(name, table, logits, B, T, y, ldy, rstd, instance_norm)
    if lens is not None and not (isinstance(lens, torch.Tensor) and lens.dtype == torch.int32 and lens.numel() == B
                                 and lens.is_contiguous()):
        raise ValueError(f"{name}: lens is a contiguous int32 tensor of B = {B} frame counts")
    if w_out is not None and not _is_f32_vec(w_out, table.J):
        raise ValueError(f"{name}: w_out is a contiguous float32 vector of {table.J} values")
    if instance_norm and T > LAYER_MIX_LDS_FRAMES and not (isinstance(stage, torch.Tensor) and stage.dtype == torch.float32
                                                            and stage.numel() >= B * T * table.H and stage.is_contiguous()):
        raise ValueError(f"{name}: more than {LAYER_MIX_LDS_FRAMES} frames need stage, contiguous float32 [B * T, H]")
    _dev(table.ptrs, logits, y, rstd, lens, w_out, stage)
    _lib.check(lib().w2v2_layer_mix_fwd(table.ptrs.data_ptr(), logits.data_ptr(), table.J, _p(lens), y.data_ptr(), ldy,
                                        _p(rstd), _p(w_out), _p(stage), B, T, table.H, int(instance_norm), dt(table._keep[0]),
                                        dt(y), stream()), name)


def layer_mix_bwd(table: LayerMixTable, logits, g, ldg: int, y, ldy: int, rstd, dm, grad_logits, workspace, B: int, T: int,
                  instance_norm: bool = True) -> None:
    """Backward of layer_mix_fwd from g = dL/dy and the stored y / rstd: dm f32 [B * T, H] (written), grad_logits f32 [J]
    (ADDED to).  Two launches, no atomics: equal inputs give equal bits."""
    name = "layer_mix_bwd"
    _mix_check(name, table, logits, B, T, g, ldg, rstd, instance_norm)
    if instance_norm:
        _mix_check(name, table, logits, B, T, y, ldy, rstd, True)
        if y.dtype != g.dtype:
            raise ValueError(f"{name}: g and y share a dtype")
    if not (isinstance(dm, torch.Tensor) and dm.dtype == torch.float32 and dm.numel() == B * T * table.H and dm.is_contiguous()):
        raise ValueError(f"{name}: dm is contiguous float32 [B * T, H]")
    if not _is_f32_vec(grad_logits, table.J):
        raise ValueError(f"{name}: grad_logits is a contiguous float32 vector of {table.J} values")
    need = 2 * B * -(-table.H // 64) * LAYER_MIX_MAX_STATES        # one f64 per workgroup and logit
    if not (isinstance(workspace, torch.Tensor) and workspace.dtype == torch.float32 and workspace.numel() >= need):
        raise ValueError(f"{name}: workspace is float32 with at least {need} values (layer_mix_workspace)")
    _dev(table.ptrs, logits, g, y, rstd, dm, grad_logits, workspace)
    _lib.check(lib().w2v2_layer_mix_bwd(table.ptrs.data_ptr(), logits.data_ptr(), table.J, g.data_ptr(), ldg, _p(y), ldy,
                                        _p(rstd), dm.data_ptr(), grad_logits.data_ptr(), workspace.data_ptr(), B, T, table.H,
                                        int(instance_norm), dt(table._keep[0]), dt(g), stream()), name)


def scale_add(G, dm, w, lo: int, hi: int, overwrite: bool) -> None:
    """G = (0 if overwrite else G) + (w[lo] + ... + w[hi]) * dm, rounded once to G's dtype; w f32 on the device (the host
    never reads it).  G f32 / bf16 / f16 and dm f32 / bf16, both contiguous with the same number of elements."""
    name = "scale_add"
    if not (isinstance(G, torch.Tensor) and isinstance(dm, torch.Tensor) and G.dtype in _MIX_X and dm.dtype in _MIX_Y):
        raise ValueError(f"{name}: G is f32 / bf16 / f16 and dm f32 / bf16")
    if G.numel() != dm.numel() or G.numel() % 8 or G.numel() == 0 or not (G.is_contiguous() and dm.is_contiguous()):
        raise ValueError(f"{name}: G and dm are contiguous with the same number of elements, a multiple of 8")
    if not (isinstance(w, torch.Tensor) and w.dtype == torch.float32 and w.dim() == 1 and w.is_contiguous()):
        raise ValueError(f"{name}: w is a contiguous float32 vector")
    if not 0 <= lo <= hi < min(w.numel(), LAYER_MIX_MAX_STATES):
        raise ValueError(f"{name}: 0 <= lo <= hi < {min(w.numel(), LAYER_MIX_MAX_STATES)}, got {lo} .. {hi}")
    if G.data_ptr() % 16 or dm.data_ptr() % 16:
        raise ValueError(f"{name}: G and dm need 16-byte aligned bases")
    _dev(G, dm, w)
    _lib.check(lib().w2v2_scale_add(G.data_ptr(), dm.data_ptr(), w.data_ptr(), lo, hi, int(bool(overwrite)), G.numel(),
                                    dt(G), dt(dm), stream()), name)


# ------------------------------------------------------------------------------------------------ heads
def row_invnorm(x, inv, rows: int, cols: int, ld: Optional[int] = None) -> None:
    _dev(x, inv)
    _lib.check(lib().w2v2_row_invnorm(x.data_ptr(), ld if ld is not None else cols, inv.data_ptr(), rows, cols,
                                      dt(x), stream()), "row_invnorm")


def aam_softmax_fwd_bwd(cos, label, softmax, loss_rows, dcos_w, dcos_x, inv_x, inv_w, rowdot, colprod, B: int,
                        Cn: int, ldc: int, margin: float, scale: float, loss_scale=None, correct_rows=None,
                        easy_margin: bool = False) -> None:
    """loss_scale: device tensor whose first element multiplies the loss gradient (fp16 loss scaling), or None.
    correct_rows [B] f32 (optional): 1 where the arg-max prediction equals the label (train_acc).
    colprod [B, Cn] f32 (optional): g * cos per element; colsum() over its rows gives the column dots."""
    _dev(cos, label, softmax, loss_rows, dcos_w, dcos_x, inv_x, inv_w, rowdot, colprod, loss_scale, correct_rows)
    dty = dt(dcos_w) if dcos_w is not None else F32
    _lib.check(lib().w2v2_aam_softmax_fwd_bwd(cos.data_ptr(), label.data_ptr(), softmax.data_ptr(),
                                              loss_rows.data_ptr(), _p(dcos_w), _p(dcos_x), _p(inv_x), _p(inv_w),
                                              _p(rowdot), _p(colprod), B, Cn, ldc, margin, scale, _p(loss_scale),
                                              _p(correct_rows), int(easy_margin), dty, stream()),
               "aam_softmax")


MARGIN_ARC, MARGIN_COS = 0, 1                 # W2V2_MARGIN_* of include/w2v2_hip.h
MARGIN_TYPES = {"arc": MARGIN_ARC, "cos": MARGIN_COS}
MARGIN_MAX_SUB_CENTERS, MARGIN_MAX_TOPK = 8, 16


def check_margin_head(C: int, K: int, n_top: int, inter_margin: float, margin_type) -> int:
    """The argument rules of w2v2_margin_softmax_fwd_bwd, on the host -> the margin type's code.  ValueError."""
    if not 1 <= int(K) <= MARGIN_MAX_SUB_CENTERS:
        raise ValueError(f"margin head: {K} sub-centres outside [1, {MARGIN_MAX_SUB_CENTERS}]")
    if not 0 <= int(n_top) <= min(C - 1, MARGIN_MAX_TOPK):
        raise ValueError(f"margin head: inter-top-k {n_top} outside [0, min({C} - 1, {MARGIN_MAX_TOPK})]")
    if not inter_margin >= 0:
        raise ValueError(f"margin head: negative inter-class margin {inter_margin}")
    mt = MARGIN_TYPES.get(margin_type, margin_type)
    if mt not in (MARGIN_ARC, MARGIN_COS):
        raise ValueError(f"margin head: margin type {margin_type!r} is neither 'arc' nor 'cos'")
    return mt


def margin_softmax_fwd_bwd(cos, label, softmax, loss_rows, dcos_w, dcos_x, inv_x, inv_w, rowdot, colprod, B: int,
                           C: int, K: int, ld: int, ldp: int, margin: float, scale: float, loss_scale=None,
                           correct_rows=None, easy_margin: bool = False, margin_type=MARGIN_ARC, n_top: int = 0,
                           inter_margin: float = 0.0) -> None:
    """The margin row pass over C classes x K adjacent sub-centre columns of cos [B, ld] (include/w2v2_hip.h "margin
    heads"): softmax [B, ldp] over the classes; the gradient of a class goes to its winning sub-centre's column of
    dcos_w / dcos_x [B, ld] and colprod [B, C * K], the other columns get zeros.  The optional tensors are those of
    aam_softmax_fwd_bwd.  margin_type: MARGIN_ARC / MARGIN_COS or "arc" / "cos".  Bad arguments: ValueError, no launch."""
    mt = check_margin_head(C, K, n_top, inter_margin, margin_type)
    if ld < C * K or ldp < C:
        raise ValueError(f"margin head: row strides {ld} / {ldp} under {C} x {K} columns / {C} classes")
    if mt == MARGIN_ARC and margin < 0:
        raise ValueError("margin head: a negative angular margin (the plain head is aam_softmax_fwd_bwd's)")
    _dev(cos, label, softmax, loss_rows, dcos_w, dcos_x, inv_x, inv_w, rowdot, colprod, loss_scale, correct_rows)
    dty = dt(dcos_w) if dcos_w is not None else F32
    _lib.check(lib().w2v2_margin_softmax_fwd_bwd(cos.data_ptr(), label.data_ptr(), softmax.data_ptr(),
                                                 loss_rows.data_ptr(), _p(dcos_w), _p(dcos_x), _p(inv_x), _p(inv_w),
                                                 _p(rowdot), _p(colprod), B, C, K, ld, ldp, margin, scale,
                                                 int(easy_margin), mt, int(n_top), inter_margin, _p(loss_scale),
                                                 _p(correct_rows), dty, stream()),
               "margin_softmax")


def normalize_bwd(g, x, inv, dot, dx, rows: int, cols: int, ldx: Optional[int] = None, add_to: bool = False) -> None:
    _dev(g, x, inv, dot, dx)
    _lib.check(lib().w2v2_normalize_bwd(g.data_ptr(), x.data_ptr(), ldx if ldx is not None else cols, inv.data_ptr(),
                                        dot.data_ptr(), dx.data_ptr(), rows, cols, dt(x), int(add_to), stream()),
               "normalize_bwd")


def aam_dw(dcos_x, emb, colprod, w_master, inv_w, dw, B: int, Cn: int, E: int, ldc: int) -> None:
    """Class-weight gradient of the AAM head (product + column dots + F.normalize backward) in one launch."""
    _dev(dcos_x, emb, colprod, w_master, inv_w, dw)
    assert emb.dtype == dcos_x.dtype and dw.dtype == torch.float32 and w_master.dtype == torch.float32
    _lib.check(lib().w2v2_aam_dw(dcos_x.data_ptr(), ldc, emb.data_ptr(), colprod.data_ptr(), w_master.data_ptr(),
                                 inv_w.data_ptr(), dw.data_ptr(), B, Cn, E, dt(emb), stream()), "aam_dw")


# ------------------------------------------------------------------------------------------------ optimiser
def adam_step(p, g, m, v, pb, n: int, lr: float, beta1: float, beta2: float, eps: float, step: int,
              grad_scale: float = 1.0, scaler=None, skip_slot: int = 0) -> None:
    """scaler: the device record of the dynamic loss scale (see grad_scaler_*), or None.  skip_slot (4 = head range,
    5 = body range of an 8-float record): the kernel takes the bias corrections at step - scaler[skip_slot], i.e. the
    number of optimiser steps that were NOT skipped for an overflow (torch GradScaler semantics)."""
    _dev(p, g, m, v, pb, scaler)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    _lib.check(lib().w2v2_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(pb),
                                    dt(pb) if pb is not None else BF16, n, lr, beta1, beta2, eps, bc1, bc2, grad_scale,
                                    _p(scaler), step, skip_slot, stream()), "adam_step")


def optim_step(algo: str, p, g, m, v, pb, n: int, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
               step: int = 1, grad_scale: float = 1.0, scaler=None, skip_slot: int = 0, weight_decay: float = 0.0,
               momentum: float = 0.0, dampening: float = 0.0, nesterov: bool = False, norm_state=None) -> None:
    """General optimiser step (w2v2_optim_step): algo "adam" (torch.optim.Adam incl. L2 weight decay) or "sgd"
    (torch.optim.SGD; the momentum buffer is ``m``, ``v`` may be None, ``m`` too without momentum).  norm_state: the
    {norm, clip_coef} record of grad_norm(), or None.  Adam without weight decay and without a record is adam_step()."""
    if algo not in ("adam", "sgd"):
        raise ValueError(f"optim_step: algo must be 'adam' or 'sgd', got {algo!r}")
    _dev(p, g, m, v, pb, scaler, norm_state)
    adam = algo == "adam"
    bc1 = 1.0 - beta1 ** step if adam else 1.0
    bc2 = 1.0 - beta2 ** step if adam else 1.0
    _lib.check(lib().w2v2_optim_step(_lib.OPTIM_ADAM if adam else _lib.OPTIM_SGD, p.data_ptr(), g.data_ptr(), _p(m), _p(v),
                                     _p(pb), dt(pb) if pb is not None else BF16, n, lr, beta1, beta2, eps, bc1, bc2,
                                     grad_scale, weight_decay, momentum, dampening, int(bool(nesterov)), _p(norm_state),
                                     _p(scaler), step, skip_slot, stream()), "optim_step")


def grad_norm_partials(n: int) -> int:
    """Doubles the partial buffer of grad_norm() needs for a slice of n elements (a pure function of n)."""
    return int(lib().w2v2_grad_norm_partials(n))


def grad_norm(g, n: int, norm_state, partials, grad_scale: float = 1.0, scaler=None, max_norm: float = 0.0) -> None:
    """norm_state (f32[2]) = {||g[:n] * grad_scale / scaler[0]||_2, min(1, max_norm / (norm + 1e-6))}: torch's
    clip_grad_norm_ after unscale_; bit-reproducible (fixed-order double sums into ``partials``, a float64 buffer).
    max_norm <= 0: norm only.  A non-finite norm sets the coefficient to 0 and scaler[1] (found_inf) to 1."""
    _dev(g, norm_state, partials, scaler)
    assert partials.dtype == torch.float64 and norm_state.dtype == torch.float32 and norm_state.numel() >= 2
    _lib.check(lib().w2v2_grad_norm(g.data_ptr(), n, grad_scale, _p(scaler), max_norm, partials.data_ptr(),
                                    partials.numel(), norm_state.data_ptr(), stream()), "grad_norm")


def grad_accumulate(acc, g, n: int, first: bool) -> None:
    """acc[:n] = g[:n] (first micro-batch of a window: acc is not read) or acc[:n] += g[:n]; f32, bit-equal to torch."""
    _dev(acc, g)
    assert acc.dtype == torch.float32 and g.dtype == torch.float32 and acc.numel() >= n and g.numel() >= n
    _lib.check(lib().w2v2_grad_accumulate(acc.data_ptr(), g.data_ptr(), n, int(bool(first)), stream()), "grad_accumulate")


def weight_residual(p, lo, table) -> None:
    """lo[off:off+n] = T(p[off:off+n] - T(p[off:off+n])) for every (off, n) row of the int64 device table."""
    _dev(p, lo, table)
    _lib.check(lib().w2v2_weight_residual(p.data_ptr(), lo.data_ptr(), table.data_ptr(), table.shape[0], dt(lo), stream()),
               "weight_residual")


def grad_scaler_check(g, n: int, state) -> None:
    """state[1] = 1 if any of g[:n] is non-finite (torch GradScaler's unscale_ / found_inf)."""
    _dev(g, state)
    _lib.check(lib().w2v2_grad_scaler_check(g.data_ptr(), n, state.data_ptr(), stream()), "grad_scaler_check")


def grad_scaler_update(state, growth: float = 2.0, backoff: float = 0.5, growth_interval: int = 2000,
                       skipped_ranges: int = 0) -> None:
    """torch GradScaler.update() on the device record {scale, found_inf, growth_tracker, skipped_steps [, skipped_head,
    skipped_body, -, -]}; skipped_ranges bit 0 / 1: this step covered the head / body range (8-float records)."""
    _dev(state)
    assert skipped_ranges == 0 or state.numel() >= 8
    _lib.check(lib().w2v2_grad_scaler_update(state.data_ptr(), growth, backoff, growth_interval, skipped_ranges, stream()),
               "grad_scaler_update")


# ------------------------------------------------------------------------------------------------ attentive pooling
def asp_context(x, ctx, B: int, T: int, C: int) -> None:
    _dev(x, ctx)
    _lib.check(lib().w2v2_asp_context(x.data_ptr(), ctx.data_ptr(), B, T, C, dt(x), stream()), "asp_context")


def asp_context_len(x, ctx, lens, B: int, T: int, C: int) -> None:
    """asp_context over the first lens[b] (device int32 [B]) frames of each utterance of x [B*T, C]."""
    _dev(x, ctx, lens)
    _lib.check(lib().w2v2_asp_context_len(x.data_ptr(), ctx.data_ptr(), lens.data_ptr(), B, T, C, dt(x), stream()),
               "asp_context_len")


def asp_context_bias(ctx, w1, b1, cb, B: int, A: int, C: int) -> None:
    _dev(ctx, w1, b1, cb)
    _lib.check(lib().w2v2_asp_context_bias(ctx.data_ptr(), w1.data_ptr(), b1.data_ptr(), cb.data_ptr(), B, A, C,
                                           stream()), "asp_context_bias")


def asp_bn_workspace(M: int, A: int, device) -> torch.Tensor:
    return torch.empty(lib().w2v2_asp_bn_workspace_floats(M, A), dtype=torch.float32, device=device)


def asp_bn_stats(a_pre, work, mean_rstd, running, M: int, A: int, eps: float, momentum: float) -> None:
    _dev(a_pre, work, mean_rstd, running)
    _lib.check(lib().w2v2_asp_bn_stats(a_pre.data_ptr(), work.data_ptr(), mean_rstd.data_ptr(), _p(running), M, A, eps,
                                       momentum, dt(a_pre), stream()), "asp_bn_stats")


def asp_bn_eval_stats(running, mean_rstd, A: int, eps: float) -> None:
    _dev(running, mean_rstd)
    _lib.check(lib().w2v2_asp_bn_eval_stats(running.data_ptr(), mean_rstd.data_ptr(), A, eps, stream()),
               "asp_bn_eval_stats")


def asp_bn_tanh(a_pre, mean_rstd, gamma, beta, h, M: int, A: int) -> None:
    _dev(a_pre, mean_rstd, gamma, beta, h)
    _lib.check(lib().w2v2_asp_bn_tanh(a_pre.data_ptr(), mean_rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                      h.data_ptr(), M, A, dt(a_pre), stream()), "asp_bn_tanh")


def asp_bn_bwd(dh, a_pre, mean_rstd, gamma, beta, work, dgamma, dbeta, da, M: int, A: int) -> None:
    _dev(dh, a_pre, mean_rstd, gamma, beta, work, dgamma, dbeta, da)
    _lib.check(lib().w2v2_asp_bn_bwd(dh.data_ptr(), a_pre.data_ptr(), mean_rstd.data_ptr(),
                                     gamma.data_ptr(), beta.data_ptr(), work.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                     da.data_ptr(), M, A, dt(dh), stream()), "asp_bn_bwd")


def asp_pool_fwd(x, s, out, stats, B: int, T: int, C: int) -> None:
    _dev(x, s, out, stats)
    _lib.check(lib().w2v2_asp_pool_fwd(x.data_ptr(), s.data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, C, dt(x),
                                       stream()), "asp_pool_fwd")


def asp_pool_fwd_len(x, s, out, stats, lens, B: int, T: int, C: int) -> None:
    """asp_pool_fwd with the softmax and the statistics over the first lens[b] (device int32 [B]) frames only."""
    _dev(x, s, out, stats, lens)
    _lib.check(lib().w2v2_asp_pool_fwd_len(x.data_ptr(), s.data_ptr(), out.data_ptr(), stats.data_ptr(), lens.data_ptr(),
                                           B, T, C, dt(x), stream()), "asp_pool_fwd_len")


def asp_pool_bwd(x, s, out, stats, dout, ds, dx, B: int, T: int, C: int) -> None:
    _dev(x, s, out, stats, dout, ds, dx)
    _lib.check(lib().w2v2_asp_pool_bwd(x.data_ptr(), s.data_ptr(), out.data_ptr(), stats.data_ptr(), dout.data_ptr(),
                                       ds.data_ptr(), dx.data_ptr(), B, T, C, dt(x), stream()), "asp_pool_bwd")


def asp_context_bwd(x, ctx, da, w1, dw1, dx, scratch, B: int, T: int, C: int, A: int) -> None:
    _dev(x, ctx, da, w1, dw1, dx, scratch)
    _lib.check(lib().w2v2_asp_context_bwd(x.data_ptr(), ctx.data_ptr(), da.data_ptr(), w1.data_ptr(), dw1.data_ptr(),
                                          dx.data_ptr(), scratch.data_ptr(), B, T, C, A, dt(x), stream()),
               "asp_context_bwd")


# ------------------------------------------------------------------------------------------------ ECAPA-TDNN pieces
def bn_workspace(M: int, C: int, device) -> torch.Tensor:
    return torch.empty(lib().w2v2_bn_workspace_floats(M, C), dtype=torch.float32, device=device)


BN_ACT_NONE, BN_ACT_RELU, BN_ACT_LEAKY = 0, 1, 2     # W2V2_BN_ACT_* (include/w2v2_hip.h); False / True are the first two


def bn_fwd(a, lda: int, work, mean_rstd, running, gamma, beta, y, ldy: int, M: int, C: int, eps: float,
           momentum: float, relu, train: bool) -> None:
    """BatchNorm1d on act(a) (``relu``: a BN_ACT_* mode, or a bool for none / ReLU): batch statistics + running update
    (train) or the running statistics."""
    _dev(a, work, mean_rstd, running, gamma, beta, y)
    _lib.check(lib().w2v2_bn_fwd(a.data_ptr(), lda, _p(work), mean_rstd.data_ptr(), _p(running), gamma.data_ptr(),
                                 beta.data_ptr(), y.data_ptr(), ldy, M, C, eps, momentum, int(relu), int(train), dt(a),
                                 stream()), "bn_fwd")


def bn_colsum_rows(M: int, C: int) -> int:
    return int(lib().w2v2_bn_colsum_rows(M, C))


def bn_bwd(dy, lddy: int, a, lda: int, mean_rstd, gamma, work, dgamma, dbeta, da, ldda: int, M: int, C: int,
           relu, colsum_partial=None, dy2=None, lddy2: int = 0) -> None:
    """colsum_partial [bn_colsum_rows(M, C), C] f32 (optional): written with the per-row-block column sums of da.
    dy2 (optional, same shape as dy, own row stride): the output gradient is dy + dy2."""
    _dev(dy, a, mean_rstd, gamma, work, dgamma, dbeta, da, colsum_partial, dy2)
    if dy2 is None:
        _lib.check(lib().w2v2_bn_bwd(dy.data_ptr(), lddy, a.data_ptr(), lda, mean_rstd.data_ptr(), gamma.data_ptr(),
                                     work.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), da.data_ptr(), ldda, M, C,
                                     int(relu), _p(colsum_partial), dt(a), stream()), "bn_bwd")
    else:
        _lib.check(lib().w2v2_bn_bwd_sum(dy.data_ptr(), lddy, dy2.data_ptr(), lddy2, a.data_ptr(), lda,
                                         mean_rstd.data_ptr(), gamma.data_ptr(), work.data_ptr(), dgamma.data_ptr(),
                                         dbeta.data_ptr(), da.data_ptr(), ldda, M, C, int(relu), _p(colsum_partial),
                                         dt(a), stream()), "bn_bwd_sum")


STAT_POOL_EPS = 1e-5          # speechbrain StatisticsPooling: added to the std


def stat_pool_fwd(x, ldx: int, out, stats, B: int, T: int, C: int, lens=None, eps: float = STAT_POOL_EPS) -> None:
    """out [B, 2C] = cat(mean_t, std_t unbiased + eps) of the f32 rows x [B * T, C] (row stride ldx); stats [B, 2C] or None:
    (mean, std) for stat_pool_bwd.  lens (device int32 [B], 2 <= lens[b] <= T): over each utterance's first lens[b] frames."""
    _dev(x, out, stats, lens)
    assert x.dtype == out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * 2 * C
    assert stats is None or (stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == B * 2 * C)
    if lens is None:
        _lib.check(lib().w2v2_stat_pool_fwd(x.data_ptr(), ldx, out.data_ptr(), _p(stats), B, T, C, eps, stream()),
                   "stat_pool_fwd")
    else:
        assert lens.dtype == torch.int32 and lens.numel() == B
        _lib.check(lib().w2v2_stat_pool_fwd_len(x.data_ptr(), ldx, out.data_ptr(), _p(stats), lens.data_ptr(), B, T, C, eps,
                                                stream()), "stat_pool_fwd_len")


def stat_pool_bwd(x, ldx: int, stats, dout, dx, lddx: int, B: int, T: int, C: int) -> None:
    """dx [B * T, C] (row stride lddx) = dmean / T + dstd (x - mean) / ((T - 1) std), dout [B, 2C] = cat(dmean, dstd); the
    second term is 0 where std = 0, as in torch."""
    _dev(x, stats, dout, dx)
    assert x.dtype == dx.dtype == stats.dtype == dout.dtype == torch.float32
    assert stats.is_contiguous() and dout.is_contiguous() and stats.numel() == dout.numel() == B * 2 * C
    _lib.check(lib().w2v2_stat_pool_bwd(x.data_ptr(), ldx, stats.data_ptr(), dout.data_ptr(), dx.data_ptr(), lddx, B, T, C,
                                        stream()), "stat_pool_bwd")


def im2col_reflect(x, ldx: int, col, B: int, T: int, Cin: int, k: int, dilation: int, x2=None, ldx2: int = 0) -> None:
    """x2 (optional, same shape, own row stride): the taps of x + x2."""
    _dev(x, col, x2)
    if x2 is None:
        _lib.check(lib().w2v2_im2col_reflect(x.data_ptr(), ldx, col.data_ptr(), B, T, Cin, k, dilation, dt(x), stream()),
                   "im2col_reflect")
    else:
        _lib.check(lib().w2v2_im2col_reflect_sum(x.data_ptr(), ldx, x2.data_ptr(), ldx2, col.data_ptr(), B, T, Cin, k,
                                                 dilation, dt(x), stream()), "im2col_reflect_sum")


def im2col_reflect_len(x, ldx: int, col, lens, B: int, T: int, Cin: int, k: int, dilation: int, x2=None,
                       ldx2: int = 0) -> None:
    """im2col_reflect of a variable-length batch: lens = device int32 [B] frame counts (padding < lens[b] <= T, checked by
    the caller); taps reflect about each utterance's own last frame, rows past it are written as zeros."""
    _dev(x, col, lens, x2)
    if x2 is None:
        _lib.check(lib().w2v2_im2col_reflect_len(x.data_ptr(), ldx, col.data_ptr(), lens.data_ptr(), B, T, Cin, k,
                                                 dilation, dt(x), stream()), "im2col_reflect_len")
    else:
        _lib.check(lib().w2v2_im2col_reflect_sum_len(x.data_ptr(), ldx, x2.data_ptr(), ldx2, col.data_ptr(),
                                                     lens.data_ptr(), B, T, Cin, k, dilation, dt(x), stream()),
                   "im2col_reflect_sum_len")


def col2im_reflect(dcol, dx, lddx: int, B: int, T: int, Cin: int, k: int, dilation: int, accumulate: bool) -> None:
    _dev(dcol, dx)
    _lib.check(lib().w2v2_col2im_reflect(dcol.data_ptr(), dx.data_ptr(), lddx, B, T, Cin, k, dilation,
                                         int(accumulate), dt(dcol), stream()), "col2im_reflect")


def add_strided(a, lda: int, b, ldb: int, y, ldy: int, M: int, C: int) -> None:
    """y = a + b over row-strided [M, C] views; b None: y = a (strided copy)."""
    _dev(a, b, y)
    _lib.check(lib().w2v2_add_strided(a.data_ptr(), lda, _p(b), ldb, y.data_ptr(), ldy, M, C, dt(a), stream()),
               "add_strided")


def copy_strided(a, lda: int, y, ldy: int, M: int, C: int) -> None:
    add_strided(a, lda, None, 0, y, ldy, M, C)


FBANK_HOP, FBANK_WIN, FBANK_TILE_FRAMES = 160, 400, 16     # (W2V2_FBANK_TILE_FRAMES of include/w2v2_hip.h)


def fbank_partial_max(B: int, T: int, device) -> torch.Tensor:
    """Workspace of fbank_db / fbank_normalize: one maximum per (utterance, tile of FBANK_TILE_FRAMES frames)."""
    return torch.empty(B, -(-T // FBANK_TILE_FRAMES), dtype=torch.float32, device=device)


def _fbank_f32(*ts) -> None:
    for t in ts:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("fbank: wav, window, fbank, db and partial_max are contiguous f32 tensors")


def fbank_db(wav, lens, window, fbank, db, partial_max) -> None:
    """wav [B, N] f32 -> db [B, 1 + N // 160, n_mels] f32 (log-mel, before the top-dB clamp) and the per-tile maxima;
    lens: device int32 [B] sample counts or None; window [400], fbank [201, n_mels]: those of data/fbank.py."""
    _dev(wav, lens, window, fbank, db, partial_max)
    _fbank_f32(wav, window, fbank, db, partial_max)
    B, N = wav.shape
    T, n_mels = 1 + N // FBANK_HOP, fbank.shape[1]
    if (window.numel() != FBANK_WIN or fbank.shape[0] != FBANK_WIN // 2 + 1 or tuple(db.shape) != (B, T, n_mels)
            or partial_max.numel() < B * -(-T // FBANK_TILE_FRAMES)
            or (lens is not None and (lens.dtype != torch.int32 or lens.numel() != B))):
        raise ValueError(f"fbank_db: shapes wav {tuple(wav.shape)}, window {tuple(window.shape)}, fbank "
                         f"{tuple(fbank.shape)}, db {tuple(db.shape)}, partial_max {tuple(partial_max.shape)}")
    _lib.check(lib().w2v2_fbank_db(wav.data_ptr(), _p(lens), window.data_ptr(), fbank.data_ptr(), db.data_ptr(),
                                   partial_max.data_ptr(), B, N, T, n_mels, stream()), "fbank_db")


def fbank_normalize(db, partial_max, lens, out, ldo: int) -> None:
    """Top-dB clamp + per-channel normalisation of fbank_db's output over each utterance's own frames into ``out`` (f32 or
    bf16, [B * T] rows of stride ldo, n_mels columns written); rows past an utterance's frames are written as zeros."""
    _dev(db, partial_max, lens, out)
    _fbank_f32(db, partial_max)
    B, T, n_mels = db.shape
    if (out.dtype not in (torch.float32, torch.bfloat16) or ldo < n_mels or out.stride(-1) != 1
            or partial_max.numel() < B * -(-T // FBANK_TILE_FRAMES)
            or out.untyped_storage().nbytes() // out.element_size() - out.storage_offset() < (B * T - 1) * ldo + n_mels
            or (lens is not None and (lens.dtype != torch.int32 or lens.numel() != B))):
        raise ValueError(f"fbank_normalize: db {tuple(db.shape)}, out {tuple(out.shape)} {out.dtype} with row stride {ldo}")
    _lib.check(lib().w2v2_fbank_normalize(db.data_ptr(), partial_max.data_ptr(), _p(lens), out.data_ptr(), ldo, dt(out),
                                          B, T, n_mels, stream()), "fbank_normalize")


def se_scale(x, g, y, B: int, T: int, C: int) -> None:
    _dev(x, g, y)
    _lib.check(lib().w2v2_se_scale(x.data_ptr(), g.data_ptr(), y.data_ptr(), B, T, C, dt(x), stream()), "se_scale")


def se_bwd_gate(dout, x, dg, B: int, T: int, C: int) -> None:
    _dev(dout, x, dg)
    _lib.check(lib().w2v2_se_bwd_gate(dout.data_ptr(), x.data_ptr(), dg.data_ptr(), B, T, C, dt(x), stream()),
               "se_bwd_gate")


def se_bwd_x(dout, g, ds, dx, B: int, T: int, C: int) -> None:
    _dev(dout, g, ds, dx)
    _lib.check(lib().w2v2_se_bwd_x(dout.data_ptr(), g.data_ptr(), ds.data_ptr(), dx.data_ptr(), B, T, C, dt(dout),
                                   stream()), "se_bwd_x")


ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2


def skinny_linear_fwd(x, W, bias, y, act: int) -> None:
    """y [B, N] = act(x [B, K] @ W [N, K]^T + bias) in exact f32 (csrc/skinny.hip)."""
    _dev(x, W, bias, y)
    assert x.dtype == W.dtype == y.dtype == torch.float32 and x.is_contiguous() and W.is_contiguous() and y.is_contiguous()
    B, K = x.shape
    N = W.shape[0]
    assert W.numel() == N * K and y.shape == (B, N)
    _lib.check(lib().w2v2_skinny_linear_fwd(x.data_ptr(), W.data_ptr(), _p(bias), y.data_ptr(), B, N, K, act, stream()),
               "skinny_linear_fwd")


def skinny_linear_bwd_x(dy, y, W, dx, act: int) -> None:
    """dx [B, K] = (dy * act'(y)) [B, N] @ W [N, K]."""
    _dev(dy, y, W, dx)
    B, N = dy.shape
    K = dx.shape[1]
    assert W.numel() == N * K and dx.shape == (B, K) and dx.is_contiguous() and dy.is_contiguous()
    _lib.check(lib().w2v2_skinny_linear_bwd_x(dy.data_ptr(), _p(y), W.data_ptr(), dx.data_ptr(), B, N, K, act, stream()),
               "skinny_linear_bwd_x")


def skinny_linear_bwd_w(dy, y, x, dW, dbias, act: int, accumulate: bool) -> None:
    """dW [N, K] (+)= (dy * act'(y))^T @ x [B, K]; dbias [N] (+)= its column sums."""
    _dev(dy, y, x, dW, dbias)
    B, N = dy.shape
    K = x.shape[1]
    assert dW.numel() == N * K and x.shape == (B, K) and x.is_contiguous() and dy.is_contiguous()
    _lib.check(lib().w2v2_skinny_linear_bwd_w(dy.data_ptr(), _p(y), x.data_ptr(), dW.data_ptr(), _p(dbias), B, N, K, act,
                                              int(accumulate), stream()), "skinny_linear_bwd_w")


def act_fwd(x, y, mode: int) -> None:
    _dev(x, y)
    _lib.check(lib().w2v2_act_fwd(x.data_ptr(), y.data_ptr(), x.numel(), mode, stream()), "act_fwd")


def act_bwd(dy, y, dx, mode: int) -> None:
    _dev(dy, y, dx)
    _lib.check(lib().w2v2_act_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), dy.numel(), mode, stream()), "act_bwd")


# ------------------------------------------------------------------------------------------------ wav2spk pieces
def _f32(*ts) -> None:
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise TypeError("the wav2spk kernels are f32 only")


def _lens(lens, B: int):
    if lens is None:
        return None
    assert lens.dtype == torch.int32 and lens.numel() == B and lens.is_cuda
    return lens.data_ptr()


def conv_out_frames(n: int, k: int, stride: int, pad: int) -> int:
    """Frames of a zero-padded strided Conv1d over n input frames (0 when the padded input is shorter than the kernel)."""
    return (n + 2 * pad - k) // stride + 1 if n + 2 * pad >= k else 0


def conv1d_first(wav, w, bias, z, ldz: int, k: int, stride: int, pad: int, lens=None) -> None:
    """z [B * T, C] (row stride ldz) = the Cin = 1 convolution of wav [B, N] with w [C, 1, k] + bias, zero padding;
    lens (device int32 [B]): SAMPLES per utterance -- samples past them count as zero, rows past the utterance's own
    frame count are written as zeros."""
    _dev(wav, w, bias, z, lens)
    _f32(wav, w, bias, z)
    B, N = wav.shape
    assert wav.stride(1) == 1 and w.is_contiguous() and w.numel() == bias.numel() * k
    _lib.check(lib().w2v2_conv1d_first(wav.data_ptr(), wav.stride(0), w.data_ptr(), bias.data_ptr(), z.data_ptr(), ldz,
                                       _lens(lens, B), B, N, conv_out_frames(N, k, stride, pad), bias.numel(), k, stride,
                                       pad, stream()), "conv1d_first")


def conv1d_first_bwd_workspace(M: int, C: int, k: int, device) -> torch.Tensor:
    return torch.empty(lib().w2v2_conv1d_first_bwd_workspace_floats(M, C, k), dtype=torch.float32, device=device)


def conv1d_first_bwd(wav, dz, lddz: int, work, dw, k: int, stride: int, pad: int) -> None:
    """dw [C, 1, k] += sum over the rows of dz [B * T, C] (row stride lddz) times the taps of wav [B, N]; fixed order."""
    _dev(wav, dz, work, dw)
    _f32(wav, dz, work, dw)
    B, N = wav.shape
    C = dw.shape[0]
    T = conv_out_frames(N, k, stride, pad)
    assert wav.stride(1) == 1 and dw.is_contiguous() and dw.numel() == C * k
    assert work.numel() >= lib().w2v2_conv1d_first_bwd_workspace_floats(B * T, C, k)
    _lib.check(lib().w2v2_conv1d_first_bwd(wav.data_ptr(), wav.stride(0), dz.data_ptr(), lddz, work.data_ptr(), dw.data_ptr(),
                                           B, N, T, C, k, stride, pad, stream()), "conv1d_first_bwd")


def im2col_zero(x, ldx: int, col, B: int, Tin: int, Cin: int, k: int, stride: int, pad: int) -> None:
    """col [B * Tout, k * Cin] (tap-major) <- x [B * Tin, Cin] (row stride ldx), zero padding."""
    _dev(x, col)
    _f32(x, col)
    Tout = conv_out_frames(Tin, k, stride, pad)
    assert col.is_contiguous() and col.numel() >= B * Tout * k * Cin
    _lib.check(lib().w2v2_im2col_zero(x.data_ptr(), ldx, col.data_ptr(), B, Tin, Tout, Cin, k, stride, pad, stream()),
               "im2col_zero")


def col2im_zero(dcol, dx, lddx: int, B: int, Tin: int, Cin: int, k: int, stride: int, pad: int) -> None:
    """dx [B * Tin, Cin] (row stride lddx, written) = the adjoint of im2col_zero applied to dcol [B * Tout, k * Cin]."""
    _dev(dcol, dx)
    _f32(dcol, dx)
    Tout = conv_out_frames(Tin, k, stride, pad)
    assert dcol.is_contiguous() and dcol.numel() >= B * Tout * k * Cin
    _lib.check(lib().w2v2_col2im_zero(dcol.data_ptr(), dx.data_ptr(), lddx, B, Tin, Tout, Cin, k, stride, pad, stream()),
               "col2im_zero")


INSTNORM_EPS = 1e-5           # torch.nn.InstanceNorm1d default


def instnorm_workspace(B: int, T: int, C: int, device) -> torch.Tensor:
    return torch.empty(lib().w2v2_instnorm_workspace_floats(B, T, C), dtype=torch.float32, device=device)


def instnorm_relu_fwd(z, ldz: int, work, mean_rstd, y, ldy: int, B: int, T: int, C: int, lens=None,
                      eps: float = INSTNORM_EPS) -> None:
    """y = relu(InstanceNorm1d(z)) over [B * T, C] rows, statistics per (utterance, channel) over time (biased variance);
    mean_rstd [B, C, 2] written.  lens (device int32 [B]): frames per utterance; rows past them are written as zeros."""
    _dev(z, work, mean_rstd, y, lens)
    _f32(z, work, mean_rstd, y)
    assert mean_rstd.is_contiguous() and mean_rstd.numel() == B * C * 2
    assert work.numel() >= lib().w2v2_instnorm_workspace_floats(B, T, C)
    _lib.check(lib().w2v2_instnorm_relu_fwd(z.data_ptr(), ldz, work.data_ptr(), mean_rstd.data_ptr(), y.data_ptr(), ldy,
                                            _lens(lens, B), B, T, C, eps, stream()), "instnorm_relu_fwd")


def instnorm_relu_bwd(dy, lddy: int, z, ldz: int, y, ldy: int, mean_rstd, work, dz, lddz: int, B: int, T: int,
                      C: int) -> None:
    """dz = the gradient of instnorm_relu_fwd's input from dy, the saved z, y and mean_rstd."""
    _dev(dy, z, y, mean_rstd, work, dz)
    _f32(dy, z, y, mean_rstd, work, dz)
    assert mean_rstd.is_contiguous() and mean_rstd.numel() == B * C * 2
    assert work.numel() >= lib().w2v2_instnorm_workspace_floats(B, T, C)
    _lib.check(lib().w2v2_instnorm_relu_bwd(dy.data_ptr(), lddy, z.data_ptr(), ldz, y.data_ptr(), ldy, mean_rstd.data_ptr(),
                                            work.data_ptr(), dz.data_ptr(), lddz, B, T, C, stream()), "instnorm_relu_bwd")


def gate_fwd(p, x, y) -> None:
    """y = sigmoid(p) * x (contiguous f32 tensors of one shape)."""
    _dev(p, x, y)
    _f32(p, x, y)
    assert p.is_contiguous() and x.is_contiguous() and y.is_contiguous() and p.numel() == x.numel() == y.numel()
    _lib.check(lib().w2v2_gate_fwd(p.data_ptr(), x.data_ptr(), y.data_ptr(), x.numel(), stream()), "gate_fwd")


def gate_bwd(dy, p, x, dp, dx) -> None:
    """dp = dy * x * s (1 - s), dx = dy * s with s = sigmoid(p)."""
    _dev(dy, p, x, dp, dx)
    _f32(dy, p, x, dp, dx)
    assert all(t.is_contiguous() and t.numel() == x.numel() for t in (dy, p, x, dp, dx))
    _lib.check(lib().w2v2_gate_bwd(dy.data_ptr(), p.data_ptr(), x.data_ptr(), dp.data_ptr(), dx.data_ptr(), x.numel(),
                                   stream()), "gate_bwd")


def sum_bias_act_rows(parts, bias, y, B: int, T: int, C: int, relu: bool, lens=None) -> None:
    """y [B * T, C] = act(bias + the sum of parts [S, B * T, C] over S, in order); lens (device int32 [B]): zeros in the rows
    past each utterance's frames.  bias None: none; y may be parts[0]."""
    _dev(parts, bias, y, lens)
    _f32(parts, bias, y)
    assert parts.is_contiguous() and y.is_contiguous() and parts.dim() == 3 and y.numel() == parts[0].numel() == B * T * C
    _lib.check(lib().w2v2_sum_bias_act_rows(parts.data_ptr(), parts.shape[0], B * T * C, _p(bias), y.data_ptr(), _lens(lens, B),
                                            B, T, C, int(relu), stream()), "sum_bias_act_rows")


def bce_head_fwd_bwd(emb, w, b, label, prob, loss_rows, dlogit, demb, dw, db, B: int, H: int, loss_scale=None) -> None:
    _dev(emb, w, b, label, prob, loss_rows, dlogit, demb, dw, db, loss_scale)
    _lib.check(lib().w2v2_bce_head_fwd_bwd(emb.data_ptr(), w.data_ptr(), b.data_ptr(), label.data_ptr(), prob.data_ptr(),
                                           loss_rows.data_ptr(), _p(dlogit), _p(demb), _p(dw), _p(db), B, H,
                                           _p(loss_scale), stream()), "bce_head")



def triplet_fwd_bwd(emb, pos, neg, d_ap, d_an, loss_rows, demb, B: int, E: int, margin: float, coef: float = 1.0,
                    accumulate: bool = False, loss_scale=None, ld: Optional[int] = None) -> None:
    """Triplet margin head (w2v2_triplet_fwd_bwd): emb [B, E] f32 with row stride ``ld`` (default emb.stride(0)), pos / neg [B] int64
    row indices on the device -> d_ap, d_an, loss_rows [B]; demb [B, E] (None = forward only) written, or added to with
    ``accumulate``, scaled by coef * loss_scale[0] / B."""
    _dev(emb, pos, neg, d_ap, d_an, loss_rows, demb, loss_scale)
    assert emb.dtype == torch.float32 and pos.dtype == torch.int64 and neg.dtype == torch.int64
    assert pos.numel() == B and neg.numel() == B and min(d_ap.numel(), d_an.numel(), loss_rows.numel()) >= B
    assert emb.dim() == 2 and emb.shape == (B, E) and emb.stride(1) == 1
    ld = emb.stride(0) if ld is None else ld
    assert ld == emb.stride(0) or B == 1, "ld must be the row stride of emb"
    assert demb is None or (demb.dtype == torch.float32 and demb.is_contiguous() and demb.numel() >= B * E)
    _lib.check(lib().w2v2_triplet_fwd_bwd(emb.data_ptr(), ld, pos.data_ptr(), neg.data_ptr(), d_ap.data_ptr(),
                                          d_an.data_ptr(), loss_rows.data_ptr(), _p(demb), B, E, float(margin), float(coef),
                                          int(bool(accumulate)), _p(loss_scale), stream()), "triplet")


CTC_MAX_TARGET = 31      # labels per utterance: 2L + 1 <= 63 extended states are one wavefront (csrc/ctc.hip)


def ctc_workspace_floats(B: int, T: int, target_width: int) -> int:
    n = lib().w2v2_ctc_workspace_floats(B, T, target_width)
    if n < 0:
        raise ValueError(f"ctc: no workspace for B = {B}, T = {T}, target width {target_width} "
                         f"(at most {CTC_MAX_TARGET} labels per utterance)")
    return int(n)


def ctc_fwd_bwd(logits, targets, input_lengths, target_lengths, loss_rows, dlogits, workspace, B: int, T: int, C: int,
                ldc: int, *, target_width: int, target_stride: Optional[int] = None, target_offset: int = 0,
                blank: int = 0, loss_scale=None) -> None:
    """CTC loss rows and d(mean loss)/d(logits) (w2v2_ctc_fwd_bwd; ref: src/optim/loss/ctc_loss.py:36-58): logits
    [B*T, ldc] f32 utterance-major, targets int64 ([B, width] rows ``target_stride`` apart; None when width is 0),
    input_lengths / target_lengths int32 [B], all on the device.  loss_rows [B] f32 = nll / max(L, 1), 0 where infinite;
    dlogits [B*T, ldc] f32 / f16 / bf16 or None (forward only).  The class of a label is label + ``target_offset``.
    workspace: f32, ``ctc_workspace_floats(B, T, target_width)`` elements."""
    _dev(logits, targets, input_lengths, target_lengths, loss_rows, dlogits, workspace, loss_scale)
    if not 0 <= target_width <= CTC_MAX_TARGET:
        raise ValueError(f"ctc: targets of width {target_width}; at most {CTC_MAX_TARGET} labels per utterance are built")
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.numel() >= B * T * ldc and ldc >= C
    assert targets is None or (targets.dtype == torch.int64 and targets.stride(-1) == 1)
    assert input_lengths.dtype == torch.int32 and target_lengths.dtype == torch.int32
    assert input_lengths.numel() == B and target_lengths.numel() == B and loss_rows.numel() >= B
    assert input_lengths.is_contiguous() and target_lengths.is_contiguous() and loss_rows.dtype == torch.float32
    assert workspace.dtype == torch.float32 and workspace.is_contiguous()
    assert dlogits is None or (dlogits.is_contiguous() and dlogits.numel() >= B * T * ldc)
    if target_stride is None:
        target_stride = target_width if targets is None or targets.dim() < 2 else targets.stride(0)
    assert targets is None or target_width == 0 or targets.numel() >= (B - 1) * target_stride + target_width
    _lib.check(lib().w2v2_ctc_fwd_bwd(logits.data_ptr(), ldc, _p(targets), target_stride, target_width, target_offset,
                                      input_lengths.data_ptr(), target_lengths.data_ptr(), blank, loss_rows.data_ptr(),
                                      _p(dlogits), _p(loss_scale), workspace.data_ptr(), workspace.numel(), B, T, C,
                                      dt(dlogits) if dlogits is not None else F32, stream()), "ctc")


CTC_LONG_MAX_TARGET = 1023      # labels per utterance of the long form: L + 1 <= 1024 threads of one workgroup (csrc/ctc_long.hip)


def ctc_long_workspace_floats(B: int, T: int, target_width: int) -> int:
    n = lib().w2v2_ctc_long_workspace_floats(B, T, target_width)
    if n < 0:
        raise ValueError(f"ctc_long: no workspace for B = {B}, T = {T}, target width {target_width} "
                         f"(at most {CTC_LONG_MAX_TARGET} labels per utterance)")
    return int(n)


def ctc_long_stage_frames(target_width: int) -> int:
    """Frames whose emissions the long lattice kernel stages in LDS at a time at this target width."""
    n = lib().w2v2_ctc_long_stage_frames(target_width)
    if n < 0:
        raise ValueError(f"ctc_long: target width {target_width} (at most {CTC_LONG_MAX_TARGET} labels per utterance)")
    return int(n)


def ctc_long_fwd_bwd(logits, targets, input_lengths, target_lengths, loss_rows, dlogits, workspace, B: int, T: int, C: int,
                     ldc: int, *, target_width: int, target_stride: Optional[int] = None, target_offset: int = 0,
                     blank: int = 0, loss_scale=None) -> None:
    """``ctc_fwd_bwd`` for transcripts (w2v2_ctc_long_fwd_bwd): the same arguments and results with up to 1023 labels per
    utterance; workspace: f32, ``ctc_long_workspace_floats(B, T, target_width)`` elements."""
    _dev(logits, targets, input_lengths, target_lengths, loss_rows, dlogits, workspace, loss_scale)
    if not 0 <= target_width <= CTC_LONG_MAX_TARGET:
        raise ValueError(f"ctc_long: targets of width {target_width}; at most {CTC_LONG_MAX_TARGET} labels per utterance "
                         "are built")
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.numel() >= B * T * ldc and ldc >= C
    assert targets is None or (targets.dtype == torch.int64 and targets.stride(-1) == 1)
    assert input_lengths.dtype == torch.int32 and target_lengths.dtype == torch.int32
    assert input_lengths.numel() == B and target_lengths.numel() == B and loss_rows.numel() >= B
    assert input_lengths.is_contiguous() and target_lengths.is_contiguous() and loss_rows.dtype == torch.float32
    assert workspace.dtype == torch.float32 and workspace.is_contiguous()
    assert dlogits is None or (dlogits.is_contiguous() and dlogits.numel() >= B * T * ldc)
    if target_stride is None:
        target_stride = target_width if targets is None or targets.dim() < 2 else targets.stride(0)
    assert targets is None or target_width == 0 or targets.numel() >= (B - 1) * target_stride + target_width
    _lib.check(lib().w2v2_ctc_long_fwd_bwd(logits.data_ptr(), ldc, _p(targets), target_stride, target_width, target_offset,
                                           input_lengths.data_ptr(), target_lengths.data_ptr(), blank,
                                           loss_rows.data_ptr(), _p(dlogits), _p(loss_scale), workspace.data_ptr(),
                                           workspace.numel(), B, T, C, dt(dlogits) if dlogits is not None else F32,
                                           stream()), "ctc_long")


def ctc_greedy_decode(logits, input_lengths, tokens, counts, B: int, T: int, C: int, ldc: int, *, blank: int = 0) -> None:
    """Greedy CTC decoding (w2v2_ctc_greedy_decode; ref: speech_recognition_module.py:233-248): logits [B*T, ldc] f32,
    input_lengths int32 [B] -> tokens int32 [B, T] (the first counts[b] of row b: argmax per frame, runs collapsed, then the
    blank dropped; the rest is not written) and counts int32 [B].  Everything on the device; one launch."""
    _dev(logits, input_lengths, tokens, counts)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.numel() >= B * T * ldc and ldc >= C
    assert input_lengths.dtype == torch.int32 and input_lengths.is_contiguous() and input_lengths.numel() == B
    assert tokens.dtype == torch.int32 and tokens.is_contiguous() and tokens.numel() >= B * T
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= B
    if not 0 <= blank < C:
        raise ValueError(f"ctc_greedy_decode: blank {blank} outside [0, {C})")
    _lib.check(lib().w2v2_ctc_greedy_decode(logits.data_ptr(), ldc, input_lengths.data_ptr(), blank, B, T, C,
                                            tokens.data_ptr(), counts.data_ptr(), stream()), "ctc_greedy_decode")


# ---------------------------------------------------------------------------------------------- trial scoring (score.hip)
STATS_CHUNK_ROWS = 128      # rows per partial of w2v2_embed_stats (csrc/score.hip ST_ROWS)
FRAME_SET_MAX_W = 256       # slots per side of w2v2_score_frame_sets (csrc/score.hip FS_MAX_W)


def _ld(t) -> int:
    """The row stride of a 2-D tensor; a one-row tensor's stride(0) is arbitrary, so at least its width."""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _bank(bank, what: str) -> Tuple[int, int, int]:
    """(rows, D, ld) of an f32 bank [rows, D] whose rows are ``ld`` elements apart; shape errors first (they need no
    device), then the device check every op makes."""
    if not isinstance(bank, torch.Tensor) or bank.dim() != 2 or bank.dtype != torch.float32:
        raise ValueError(f"{what}: the bank is a 2-D float32 tensor")
    rows, D = bank.shape
    ld = _ld(bank)
    if rows < 1 or D < 4 or D % 4 != 0:
        raise ValueError(f"{what}: D = {D} must be a positive multiple of 4 (and the bank non-empty)")
    if bank.stride(1) != 1 or ld < D or ld % 4 != 0 or bank.data_ptr() % 16 != 0:
        raise ValueError(f"{what}: row stride ld = {ld} must be >= D = {D} and a multiple of 4, features contiguous, "
                         "base 16-byte aligned")
    return rows, D, ld


def _out(t, n: int, device, what: str, name: str, dtype=torch.float32) -> torch.Tensor:
    """An optional output of n elements: checked when given, allocated on ``device`` otherwise."""
    if t is None:
        return torch.empty(n, dtype=dtype, device=device)
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or t.numel() < n:
        raise ValueError(f"{what}: {name} is a contiguous {str(dtype).replace('torch.', '')} tensor of at least {n} elements")
    return t


def _pairs(pairs, what: str) -> int:
    """P of a trial table: device int32 [P, 2].  The row numbers are not read here (the kernels answer a bad one with NaN)."""
    if not isinstance(pairs, torch.Tensor) or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 \
            or pairs.shape[0] < 1 or not pairs.is_contiguous():
        raise ValueError(f"{what}: pairs is a contiguous int32 [P, 2] tensor, P >= 1")
    return pairs.shape[0]


def _centring(mean, std, D: int, what: str) -> None:
    if (mean is None) != (std is None):
        raise ValueError(f"{what}: mean and std are given together or not at all")
    for v in (mean, std):
        if v is not None and (not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.shape != (D,)
                              or not v.is_contiguous()):
            raise ValueError(f"{what}: mean / std are contiguous float32 [{D}]")


def embed_stats_workspace(N: int, D: int, device) -> torch.Tensor:
    return torch.empty(2 * ((N + STATS_CHUNK_ROWS - 1) // STATS_CHUNK_ROWS) * D, dtype=torch.float64, device=device)


def embed_stats(bank, mean_out=None, std_out=None, workspace=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-dimension mean and unbiased std of bank [N, D] (w2v2_embed_stats = torch.std_mean(bank, dim=0), the evaluator's
    compute_mean_std_batch) -> (mean [D], std [D]) on the device.  Two launches, sums in double."""
    N, D, ld = _bank(bank, "embed_stats")
    if N < 2:
        raise ValueError(f"embed_stats: the unbiased std needs N >= 2 rows (got {N})")
    _dev(bank, mean_out, std_out, workspace)
    mean_out = _out(mean_out, D, bank.device, "embed_stats", "mean_out")
    std_out = _out(std_out, D, bank.device, "embed_stats", "std_out")
    if workspace is None:
        workspace = embed_stats_workspace(N, D, bank.device)
    need = embed_stats_workspace(N, D, "meta").numel()
    if workspace.dtype != torch.float64 or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"embed_stats: workspace holds {need} float64 (embed_stats_workspace)")
    _lib.check(lib().w2v2_embed_stats(bank.data_ptr(), ld, N, D, mean_out.data_ptr(), std_out.data_ptr(),
                                      workspace.data_ptr(), stream()), "embed_stats")
    return mean_out, std_out


def score_pairs(bank, pairs, mean=None, std=None, length_norm: bool = False, cos_out=None,
                score_out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Cosine score of the trials pairs [P, 2] (device int32 rows of bank [N, D]) -> (cos [P], score [P]) with
    score = clamp((cos + 1) / 2, 0, 1); mean / std [D] (both or neither): z-score first; length_norm: F.normalize first
    (w2v2_score_pairs).  The indices are NOT checked here (they are on the device: a trial with an index outside [0, N)
    comes back NaN); TrialIndex checks a list before it is uploaded."""
    N, D, ld = _bank(bank, "score_pairs")
    _centring(mean, std, D, "score_pairs")
    P = _pairs(pairs, "score_pairs")
    _dev(bank, pairs, mean, std, cos_out, score_out)
    cos_out = _out(cos_out, P, bank.device, "score_pairs", "cos_out")
    score_out = _out(score_out, P, bank.device, "score_pairs", "score_out")
    _lib.check(lib().w2v2_score_pairs(bank.data_ptr(), ld, N, D, pairs.data_ptr(), P, _p(mean), _p(std),
                                      int(bool(length_norm)), cos_out.data_ptr(), score_out.data_ptr(), stream()),
               "score_pairs")
    return cos_out, score_out


def score_frame_sets(frames, sel, counts, cos_out=None, score_out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The non-pooled score (w2v2_score_frame_sets): frames [rows, D] a ragged frame bank, sel [P, 2, W] device int32
    absolute row numbers (left side, right side), counts [P, 2] device int32 the slots used -> (cos [P], score [P]), cos =
    the mean of all pairwise frame cosines.  A count outside [1, W] or a row outside [0, rows) gives NaN for that trial."""
    rows, D, ld = _bank(frames, "score_frame_sets")
    if not isinstance(sel, torch.Tensor) or sel.dtype != torch.int32 or sel.dim() != 3 or sel.shape[1] != 2 \
            or sel.shape[0] < 1 or not 1 <= sel.shape[2] <= FRAME_SET_MAX_W or not sel.is_contiguous():
        raise ValueError(f"score_frame_sets: sel is a contiguous int32 [P, 2, W] tensor, 1 <= W <= {FRAME_SET_MAX_W}")
    P, _, W = sel.shape
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.shape != (P, 2) \
            or not counts.is_contiguous():
        raise ValueError(f"score_frame_sets: counts is a contiguous int32 [{P}, 2] tensor")
    _dev(frames, sel, counts, cos_out, score_out)
    cos_out = _out(cos_out, P, frames.device, "score_frame_sets", "cos_out")
    score_out = _out(score_out, P, frames.device, "score_frame_sets", "score_out")
    _lib.check(lib().w2v2_score_frame_sets(frames.data_ptr(), ld, rows, D, sel.data_ptr(), counts.data_ptr(), W, P,
                                           cos_out.data_ptr(), score_out.data_ptr(), stream()), "score_frame_sets")
    return cos_out, score_out


# ---------------------------------------------------------------------------------------------- score normalisation (score_norm.hip)
TOPK_LDS_KEYS = 8192                    # longest row w2v2_topk_stats stages in LDS (csrc/score_norm.hip TK_LDS_KEYS)
TOPK_MAX_M = 2 ** 24                    # M of w2v2_topk_stats stays below this
SCORE_NORM_MODES = {"z": 0, "t": 1, "s": 2}
COHORT_WORKSPACE_BYTES = 256 << 20      # the default block of cohort_stats keeps its [rows_per_block, ldS] buffer at or below this


def _top_k(K, M: int, what: str) -> int:
    if isinstance(K, bool) or not isinstance(K, int) or not 2 <= K <= M:
        raise ValueError(f"{what}: K = {K!r} outside [2, M = {M}]")
    return K


def rows_transform(x, mean=None, std=None, length_norm: bool = False, out=None,
                   inv_norm=None) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """The evaluator's transform of the rows of x [rows, D] (w2v2_rows_transform: z-score with mean / std, then
    F.normalize with length_norm, as w2v2_score_pairs applies them) -> (u [rows, D], inv_norm [rows] = 1 / max(|u|, 1e-8)).
    Without centring and length norm nothing is copied: u is None (the rows are their own transform) and only inv_norm is
    written, unless ``out`` is given."""
    rows, D, ld = _bank(x, "rows_transform")
    _centring(mean, std, D, "rows_transform")
    plain = mean is None and not length_norm
    if out is not None:
        orows, oD, old = _bank(out, "rows_transform (out)")
        if oD != D or orows < rows:
            raise ValueError(f"rows_transform: out is float32 [{rows}, {D}]")
    _dev(x, mean, std, out, inv_norm)
    if out is None and not plain:
        out = torch.empty(rows, D, dtype=torch.float32, device=x.device)
    inv_norm = _out(inv_norm, rows, x.device, "rows_transform", "inv_norm")
    _lib.check(lib().w2v2_rows_transform(x.data_ptr(), ld, rows, D, _p(mean), _p(std), int(bool(length_norm)), _p(out),
                                         0 if out is None else _ld(out), inv_norm.data_ptr(), stream()), "rows_transform")
    return (None if out is None else out[:rows]), inv_norm


def topk_stats(S, K: int, M: Optional[int] = None, mu_out=None, sd_out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Mean and unbiased std of the K largest of the first M values of every row of S [R, ldS] f32 (w2v2_topk_stats; M
    defaults to the row length) -> (mu [R], sd [R]).  Exact selection, ties counted as a multiset, -0.0 = +0.0; a row with
    a NaN gives NaN for that row.  2 <= K <= M < 2^24."""
    if not isinstance(S, torch.Tensor) or S.dim() != 2 or S.dtype != torch.float32 or S.shape[0] < 1:
        raise ValueError("topk_stats: S is a 2-D float32 tensor")
    R = S.shape[0]
    M = S.shape[1] if M is None else int(M)
    ldS = _ld(S)
    if not 2 <= M <= S.shape[1] or M >= TOPK_MAX_M:
        raise ValueError(f"topk_stats: M = {M} outside [2, min({S.shape[1]} columns, 2^24 - 1)]")
    if S.stride(1) != 1 or ldS % 4 != 0 or S.data_ptr() % 16 != 0:
        raise ValueError(f"topk_stats: row stride ldS = {ldS} must be a multiple of 4, values contiguous, base 16-byte aligned")
    K = _top_k(K, M, "topk_stats")
    _dev(S, mu_out, sd_out)
    mu_out = _out(mu_out, R, S.device, "topk_stats", "mu_out")
    sd_out = _out(sd_out, R, S.device, "topk_stats", "sd_out")
    _lib.check(lib().w2v2_topk_stats(S.data_ptr(), ldS, R, M, K, mu_out.data_ptr(), sd_out.data_ptr(), stream()), "topk_stats")
    return mu_out, sd_out


def score_pairs_norm(cos, pairs, mu, sd, mode: str = "s", score_out=None) -> torch.Tensor:
    """The normalised score of the trials pairs [P, 2] (device int32) with raw cosines cos [P] and the cohort statistics
    mu / sd [N] (w2v2_score_pairs_norm): z_e = (c - mu[e]) / (sd[e] + 1e-12), z_t likewise; mode "z" -> z_e, "t" -> z_t,
    "s" -> their mean.  Unbounded: not mapped to [0, 1].  An index outside [0, N) gives NaN for that trial."""
    if mode not in SCORE_NORM_MODES:
        raise ValueError(f"score_pairs_norm: mode={mode!r}: 'z', 't' or 's'")
    P = _pairs(pairs, "score_pairs_norm")
    if not isinstance(cos, torch.Tensor) or cos.dtype != torch.float32 or cos.dim() != 1 or cos.numel() != P \
            or not cos.is_contiguous():
        raise ValueError(f"score_pairs_norm: cos is a contiguous float32 [{P}] tensor")
    for v in (mu, sd):
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.dim() != 1 or v.numel() < 1 \
                or not v.is_contiguous() or v.shape != mu.shape:
            raise ValueError("score_pairs_norm: mu / sd are contiguous float32 [N] tensors")
    _dev(cos, pairs, mu, sd, score_out)
    score_out = _out(score_out, P, cos.device, "score_pairs_norm", "score_out")
    _lib.check(lib().w2v2_score_pairs_norm(cos.data_ptr(), pairs.data_ptr(), P, mu.data_ptr(), sd.data_ptr(), mu.numel(),
                                           SCORE_NORM_MODES[mode], score_out.data_ptr(), stream()), "score_pairs_norm")
    return score_out


def segment_mean(bank, order, offsets, out=None) -> torch.Tensor:
    """Mean of the bank rows of every segment (w2v2_segment_mean): bank [N, D] f32, order int32 [N] the rows grouped by
    segment, offsets int32 [S + 1] -> out [S, D].  order and offsets are device tensors built on the host
    (evaluation.speaker.device_scoring.speaker_mean_cohort checks them there: a permutation, no empty segment)."""
    N, D, ld = _bank(bank, "segment_mean")
    if not isinstance(order, torch.Tensor) or order.dtype != torch.int32 or order.shape != (N,) or not order.is_contiguous():
        raise ValueError(f"segment_mean: order is a contiguous int32 [{N}] tensor")
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int32 or offsets.dim() != 1 \
            or not 2 <= offsets.numel() <= N + 1 or not offsets.is_contiguous():
        raise ValueError(f"segment_mean: offsets is a contiguous int32 [S + 1] tensor, 1 <= S <= N = {N}")
    S = offsets.numel() - 1
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != (S, D)
                            or not out.is_contiguous()):
        raise ValueError(f"segment_mean: out is a contiguous float32 [{S}, {D}] tensor")
    _dev(bank, order, offsets, out)
    if out is None:
        out = torch.empty(S, D, dtype=torch.float32, device=bank.device)
    _lib.check(lib().w2v2_segment_mean(bank.data_ptr(), ld, N, D, order.data_ptr(), offsets.data_ptr(), S, out.data_ptr(), D,
                                       stream()), "segment_mean")
    return out


def cohort_rows_per_block(N: int, M: int) -> int:
    """Bank rows per block of cohort_stats by default: the [rows, ldS] f32 buffer stays at or below 256 MiB."""
    return max(1, min(int(N), COHORT_WORKSPACE_BYTES // (4 * ((int(M) + 3) // 4 * 4))))


def cohort_stats(bank, cohort, K: int, mean=None, std=None, length_norm: bool = False, rows_per_block: Optional[int] = None,
                 workspace=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The cohort statistics of every bank row (steps 1-3 of include/w2v2_hip.h, "score normalisation"): bank [N, D] and
    cohort [M, D] go through the evaluator's transform, every bank row is scored against every cohort row
    (S = U C^T on the exact-f32 MFMA GEMM with the two inverse norms as row / column scales) and the K largest cosines
    of each row give (mu [N], sd [N]) on the device.  S is never held whole: the bank goes in blocks of ``rows_per_block``
    rows through one ``workspace`` of at least rows_per_block * ldS float32 (ldS = M rounded up to 4)."""
    N, D, _ = _bank(bank, "cohort_stats")
    M, Dc, _ = _bank(cohort, "cohort_stats (cohort)")
    if Dc != D:
        raise ValueError(f"cohort_stats: the cohort has D = {Dc}, the bank D = {D}")
    if M >= TOPK_MAX_M:
        raise ValueError(f"cohort_stats: M = {M} cohort rows, at most 2^24 - 1")
    K = _top_k(K, M, "cohort_stats")
    _centring(mean, std, D, "cohort_stats")
    ldS = (M + 3) // 4 * 4
    if rows_per_block is None:
        rows_per_block = cohort_rows_per_block(N, M)
    if isinstance(rows_per_block, bool) or not isinstance(rows_per_block, int) or rows_per_block < 1:
        raise ValueError(f"cohort_stats: rows_per_block = {rows_per_block!r} must be a positive integer")
    rpb = min(rows_per_block, N)
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float32
                                  or not workspace.is_contiguous() or workspace.numel() < rpb * ldS
                                  or workspace.data_ptr() % 16 != 0):
        raise ValueError(f"cohort_stats: workspace holds rows_per_block * ldS = {rpb} * {ldS} float32, contiguous, 16-byte "
                         "aligned")
    _dev(bank, cohort, mean, std, workspace)
    dev = bank.device
    if workspace is None:
        workspace = torch.empty(rpb * ldS, dtype=torch.float32, device=dev)
    S = workspace.view(-1)[:rpb * ldS].view(rpb, ldS)
    plain = mean is None and not length_norm
    c_u, c_inv = rows_transform(cohort, mean, std, length_norm)
    c_u = cohort if c_u is None else c_u
    u_buf = None if plain else torch.empty(rpb, D, dtype=torch.float32, device=dev)
    inv_buf = torch.empty(rpb, dtype=torch.float32, device=dev)
    mu = torch.empty(N, dtype=torch.float32, device=dev)
    sd = torch.empty(N, dtype=torch.float32, device=dev)
    for r0 in range(0, N, rpb):
        rows = min(rpb, N - r0)
        blk = bank[r0:r0 + rows]
        u, inv = rows_transform(blk, mean, std, length_norm, out=u_buf, inv_norm=inv_buf)
        u = blk if u is None else u
        Gemm(rows, M, D, u, c_u, S, lda=_ld(u), ldb=_ld(c_u), ldc=ldS, epilogue=EPI_SCALE_RC, row_scale=inv, col_scale=c_inv)()
        topk_stats(S[:rows], K, M, mu[r0:r0 + rows], sd[r0:r0 + rows])
    return mu, sd


# ---------------------------------------------------------------------------------------------- scoring back-ends (backend.hip)
SCATTER_ROWS_PER_BLOCK = 4096           # rows of one f32 block product of class_scatter by default
SCATTER_BLOCKS_PER_LAUNCH = 4           # block products of one batched GEMM launch: a [D, D] product alone is 144 tiles at D = 1,536


def _row_vector(t, rows: int, dtype, what: str, name: str) -> None:
    if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dtype or t.shape != (rows,) or not t.is_contiguous()):
        raise ValueError(f"{what}: {name} is a contiguous {str(dtype).replace('torch.', '')} [{rows}] tensor")


def rows_center(x, means, seg_id=None, row_weight=None, out=None) -> torch.Tensor:
    """out[r] = w_r * (x[r] - means[seg_id[r]]) (w2v2_rows_center): x [rows, D] f32, means [S, D] f32, seg_id device int32
    [rows] or None (every row takes means[0]), row_weight f32 [rows] or None (w = 1) -> out [rows, D].  One subtraction
    and one multiplication in f32 per element.  seg_id is NOT checked here (it is on the device: a row whose id lies
    outside [0, S) comes back NaN)."""
    rows, D, ld = _bank(x, "rows_center")
    S, Dm, ldm = _bank(means, "rows_center (means)")
    if Dm != D:
        raise ValueError(f"rows_center: means has D = {Dm}, the rows D = {D}")
    _row_vector(seg_id, rows, torch.int32, "rows_center", "seg_id")
    _row_vector(row_weight, rows, torch.float32, "rows_center", "row_weight")
    if out is not None:
        orows, oD, _ = _bank(out, "rows_center (out)")
        if oD != D or orows < rows or out.data_ptr() == x.data_ptr():
            raise ValueError(f"rows_center: out is float32 [{rows}, {D}], not the input")
    _dev(x, means, seg_id, row_weight, out)
    if out is None:
        out = torch.empty(rows, D, dtype=torch.float32, device=x.device)
    _lib.check(lib().w2v2_rows_center(x.data_ptr(), ld, rows, D, _p(seg_id), means.data_ptr(), ldm, S, _p(row_weight),
                                      out.data_ptr(), _ld(out), stream()), "rows_center")
    return out[:rows]


def scatter_fold(block, acc, first: bool) -> torch.Tensor:
    """acc = (0 if first else acc) + block (w2v2_scatter_fold): block [D, D] f32 (row stride a multiple of 4), acc a
    contiguous float64 [D, D] on the device.  With ``first`` acc is not read."""
    D, D2, ldb = _bank(block, "scatter_fold")
    if D2 != D:
        raise ValueError(f"scatter_fold: block is square (got [{D}, {D2}])")
    if not isinstance(acc, torch.Tensor) or acc.dtype != torch.float64 or acc.shape != (D, D) or not acc.is_contiguous() \
            or acc.data_ptr() % 16 != 0:
        raise ValueError(f"scatter_fold: acc is a contiguous float64 [{D}, {D}] tensor, 16-byte aligned")
    _dev(block, acc)
    _lib.check(lib().w2v2_scatter_fold(block.data_ptr(), ldb, acc.data_ptr(), D, int(bool(first)), stream()), "scatter_fold")
    return acc


def plda_score_pairs(u, pairs, p, q, k: float, llr_out=None) -> torch.Tensor:
    """The PLDA log-likelihood ratio of the trials pairs [P, 2] (device int32 rows of the diagonalised bank u [N, Q] f32)
    -> llr [P] f32: k + sum_d p_d u_e,d u_t,d - sum_d q_d (u_e,d^2 + u_t,d^2), every product and sum in double
    (w2v2_plda_score_pairs).  p, q: contiguous float64 [Q] on the device; k a host float.  Unbounded.  The indices are NOT
    checked here: a trial with an index outside [0, N) comes back NaN."""
    N, Q, ld = _bank(u, "plda_score_pairs")
    P = _pairs(pairs, "plda_score_pairs")
    for v in (p, q):
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float64 or v.shape != (Q,) or not v.is_contiguous() \
                or v.data_ptr() % 16 != 0:
            raise ValueError(f"plda_score_pairs: p / q are contiguous float64 [{Q}] tensors, 16-byte aligned")
    _dev(u, pairs, p, q, llr_out)
    llr_out = _out(llr_out, P, u.device, "plda_score_pairs", "llr_out")
    _lib.check(lib().w2v2_plda_score_pairs(u.data_ptr(), ld, N, Q, pairs.data_ptr(), P, p.data_ptr(), q.data_ptr(), float(k),
                                           llr_out.data_ptr(), stream()), "plda_score_pairs")
    return llr_out


def class_scatter_workspace(N: int, D: int, rows_per_block: int = SCATTER_ROWS_PER_BLOCK) -> int:
    """float32 elements of the workspace of class_scatter: the centred blocks of one launch and their products."""
    rpb = min(int(rows_per_block), int(N))
    g = max(1, min(SCATTER_BLOCKS_PER_LAUNCH, int(N) // rpb))
    return g * (rpb * int(D) + int(D) * int(D))


def class_scatter(bank, seg_id, means, row_weight=None, rows_per_block: int = SCATTER_ROWS_PER_BLOCK,
                  workspace=None) -> torch.Tensor:
    """sum_r a_r a_r^T with a_r = w_r (bank[r] - means[seg_id[r]]) -> float64 [D, D] on the device (step 1 of
    include/w2v2_hip.h, "scoring back-ends"): the bank goes in blocks of at most ``rows_per_block`` rows through
    rows_center, the exact-f32 MFMA GEMM (A^T A in f32, one product per block, up to SCATTER_BLOCKS_PER_LAUNCH of them in
    one batched launch) and scatter_fold (the f64 accumulator), blocks in ascending order.
    seg_id device int32 [N] or None (one mean row), row_weight f32 [N] or None.  The result is not symmetrised (the two
    triangles may differ in the last f32 bits of a block product); ``workspace``: class_scatter_workspace float32."""
    N, D, _ = _bank(bank, "class_scatter")
    S, Dm, _ = _bank(means, "class_scatter (means)")
    if Dm != D:
        raise ValueError(f"class_scatter: means has D = {Dm}, the bank D = {D}")
    _row_vector(seg_id, N, torch.int32, "class_scatter", "seg_id")
    _row_vector(row_weight, N, torch.float32, "class_scatter", "row_weight")
    if isinstance(rows_per_block, bool) or not isinstance(rows_per_block, int) or rows_per_block < 1:
        raise ValueError(f"class_scatter: rows_per_block = {rows_per_block!r} must be a positive integer")
    rpb = min(rows_per_block, N)
    need = class_scatter_workspace(N, D, rpb)
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.float32
                                  or not workspace.is_contiguous() or workspace.numel() < need
                                  or workspace.data_ptr() % 16 != 0):
        raise ValueError(f"class_scatter: workspace holds {need} float32 (class_scatter_workspace), contiguous, 16-byte aligned")
    _dev(bank, seg_id, means, row_weight, workspace)
    dev = bank.device
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=dev)
    full = N // rpb                                     # whole blocks; the rows behind them are one more, shorter block
    G = max(1, min(SCATTER_BLOCKS_PER_LAUNCH, full))
    a_buf = workspace.view(-1)[:G * rpb * D].view(G * rpb, D)
    prod = workspace.view(-1)[G * rpb * D:G * (rpb * D + D * D)].view(G, D, D)
    acc = torch.empty(D, D, dtype=torch.float64, device=dev)
    products = {}
    r0 = 0
    while r0 < N:
        g = min(G, (N - r0) // rpb)                     # blocks of this launch: up to G whole ones, or the last short one
        k = rpb if g else N - r0
        g = max(g, 1)
        rows = g * k
        rows_center(bank[r0:r0 + rows], means, None if seg_id is None else seg_id[r0:r0 + rows],
                    None if row_weight is None else row_weight[r0:r0 + rows], out=a_buf)
        if (g, k) not in products:                      # (at most three shapes: G blocks, fewer blocks, the short block)
            products[g, k] = Gemm(D, D, k, a_buf, a_buf, prod, lda=D, ldb=D, ldc=D, transA=True, transB=True, batch=g,
                                  a_strides=(k * D, 0), b_strides=(k * D, 0), c_strides=(D * D, 0))
        products[g, k]()
        for z in range(g):                              # the fold keeps the blocks in ascending order
            scatter_fold(prod[z], acc, first=r0 == 0 and z == 0)
        r0 += rows
    return acc


# ---------------------------------------------------------------------------------------------- trial metrics (metrics.hip)
SORT_TILE = 2048           # keys per workgroup per pass of w2v2_sort_f32_index (csrc/metrics.hip SORT_TILE)
TRIAL_METRICS_FIELDS = ("eer", "eer_threshold", "mdc", "mdc_threshold", "n_pos", "n_neg", "n_nan", "n_thresholds")


def _trial_count(t, dtype, what: str, name: str) -> int:
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != dtype or not t.is_contiguous() or t.numel() < 1:
        raise ValueError(f"{what}: {name} is a contiguous 1-D {str(dtype).replace('torch.', '')} tensor of P >= 1 elements")
    if t.numel() >= 2 ** 31:
        raise ValueError(f"{what}: P = {t.numel()} must be below 2^31")
    return t.numel()


def _labels(labels, P: int, what: str, unit: str) -> None:
    if _trial_count(labels, torch.uint8, what, "labels") != P:
        raise ValueError(f"{what}: one label per {unit} (P = {P})")


def cost_checks(c_miss, c_fa, p_target, open_prior: bool = False) -> None:
    """The operating point of a detection cost, with calculate_mdc's own errors (ref: src/eval_metrics.py:90-206);
    ``open_prior``: a fit also needs finite prior log-odds.  evaluation.speaker.calibration checks with this as well."""
    if c_miss < 1:
        raise ValueError(f"c_miss={c_miss} should be >= 1")
    if c_fa < 1:
        raise ValueError(f"c_fa={c_fa} should be >= 1")
    if p_target < 0 or p_target > 1:
        raise ValueError(f"p_target={p_target} should be between 0 and 1")
    if open_prior and (p_target == 0 or p_target == 1):
        raise ValueError(f"p_target={p_target} should be strictly between 0 and 1: the prior log-odds must be finite")


def _byte_workspace(workspace, need: int, device, what: str, sizer: str) -> torch.Tensor:
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need \
            or workspace.data_ptr() % 16 != 0:
        raise ValueError(f"{what}: workspace holds {need} bytes, uint8, 16-byte aligned ({sizer})")
    return workspace


def _workspace_bytes(entry: str, P: int) -> int:
    if not 1 <= int(P) < 2 ** 31:
        raise ValueError(f"{entry}: P = {P} outside [1, 2^31)")
    return int(getattr(lib(), entry)(int(P)))


def sort_f32_index_workspace(P: int, device) -> torch.Tensor:
    return torch.empty(_workspace_bytes("w2v2_sort_f32_index_workspace_bytes", P), dtype=torch.uint8, device=device)


def sort_f32_index(keys, order_out=None, keys_out=None, workspace=None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Stable ascending argsort of keys [P] f32 on the device (w2v2_sort_f32_index) -> (order int32 [P], keys_out): order
    equals np.argsort(keys, kind="stable") exactly (-0.0 ties with +0.0, NaNs behind +inf in index order); keys_out (when
    given) receives keys[order].  The order the host metrics take with two argsorts (ref: src/eval_metrics.py:54-79 through
    roc_curve, :90-206)."""
    P = _trial_count(keys, torch.float32, "sort_f32_index", "keys")
    order_out = _out(order_out, P, keys.device, "sort_f32_index", "order_out", torch.int32)
    if keys_out is not None:                            # (not allocated: without it the sorted keys are not written)
        _out(keys_out, P, keys.device, "sort_f32_index", "keys_out")
    _dev(keys, order_out, keys_out, workspace)
    workspace = _byte_workspace(workspace, _workspace_bytes("w2v2_sort_f32_index_workspace_bytes", P), keys.device,
                                "sort_f32_index", "sort_f32_index_workspace")
    _lib.check(lib().w2v2_sort_f32_index(keys.data_ptr(), P, order_out.data_ptr(), _p(keys_out), workspace.data_ptr(),
                                         stream()), "sort_f32_index")
    return order_out, keys_out


def trial_metrics_workspace(P: int, device) -> torch.Tensor:
    return torch.empty(_workspace_bytes("w2v2_trial_metrics_workspace_bytes", P), dtype=torch.uint8, device=device)


def trial_metrics(scores, labels, c_miss=1, c_fa=1, p_target=0.05, out=None, workspace=None) -> torch.Tensor:
    """EER / minDCF of scores [P] f32 and labels [P] uint8 (0 / 1), both on the device (w2v2_trial_metrics; ref:
    src/eval_metrics.py:54-79 calculate_eer, :90-206 calculate_mdc) -> out [8] float64 on the device, in the order of
    TRIAL_METRICS_FIELDS.  With NaN scores (n_nan > 0) or one class absent the
    other fields are unspecified: evaluation.speaker.device_scoring.metrics_device answers those on the host."""
    cost_checks(c_miss, c_fa, p_target)
    P = _trial_count(scores, torch.float32, "trial_metrics", "scores")
    _labels(labels, P, "trial_metrics", "score")
    out = _out(out, 8, scores.device, "trial_metrics", "out", torch.float64)
    _dev(scores, labels, out, workspace)
    workspace = _byte_workspace(workspace, _workspace_bytes("w2v2_trial_metrics_workspace_bytes", P), scores.device,
                                "trial_metrics", "trial_metrics_workspace")
    _lib.check(lib().w2v2_trial_metrics(scores.data_ptr(), labels.data_ptr(), P, float(c_miss), float(c_fa), float(p_target),
                                        out.data_ptr(), workspace.data_ptr(), stream()), "trial_metrics")
    return out


# ------------------------------------------------------------------------------------------ score calibration (calibration.hip)
# include/w2v2_hip.h "score calibration" is the definition; evaluation/speaker/calibration.py is the user's side.
CALIB_TILE = 2048          # trials per workgroup of w2v2_calib_fit / w2v2_llr_metrics (csrc/calibration.hip CAL_TILE)
CALIB_MAX_SYSTEMS = 8      # W2V2_CALIB_MAX_SYSTEMS
CALIB_RECORD_DOUBLES = 168  # w2v2_calib_record_doubles()
CALIB_STATUS = {0: "running", 1: "converged", 2: "failed", 3: "small step"}
LLR_METRICS_FIELDS = ("cllr", "cllr_tar", "cllr_non", "act_dcf", "act_p_miss", "act_p_fa", "n_pos", "n_nan")
_CALIB_N = CALIB_MAX_SYSTEMS + 1
# name -> (first double, count) of the record
CALIB_RECORD = {"status": (0, 1), "rounds": (1, 1), "K": (2, 1), "J": (3, 1), "step": (4, 1), "decrement": (5, 1),
                "n_tar": (6, 1), "n_non": (7, 1), "n_nan": (8, 1), "J_trial": (9, 1),
                "w": (16, _CALIB_N), "d": (16 + _CALIB_N, _CALIB_N), "w_trial": (16 + 2 * _CALIB_N, _CALIB_N),
                "mean": (16 + 3 * _CALIB_N, CALIB_MAX_SYSTEMS), "sd": (16 + 3 * _CALIB_N + CALIB_MAX_SYSTEMS, CALIB_MAX_SYSTEMS),
                "r": (16 + 3 * _CALIB_N + 2 * CALIB_MAX_SYSTEMS, CALIB_MAX_SYSTEMS),
                "a": (16 + 3 * _CALIB_N + 3 * CALIB_MAX_SYSTEMS, _CALIB_N),
                "g": (16 + 4 * _CALIB_N + 3 * CALIB_MAX_SYSTEMS, _CALIB_N),
                "H": (16 + 5 * _CALIB_N + 3 * CALIB_MAX_SYSTEMS, _CALIB_N * _CALIB_N)}


def calib_record_fields(record) -> dict:
    """One host copy of a fit's record (any sequence of CALIB_RECORD_DOUBLES numbers) -> its fields by name: scalars as
    floats (status, rounds and K as ints), vectors cut to K (+ 1) elements, H as a [K + 1][K + 1] list."""
    rec = [float(v) for v in (record.cpu().tolist() if isinstance(record, torch.Tensor) else record)]
    if len(rec) < CALIB_RECORD_DOUBLES:
        raise ValueError(f"calib_record_fields: a record has {CALIB_RECORD_DOUBLES} doubles")
    K = int(rec[2])
    out = {}
    for name, (at, n) in CALIB_RECORD.items():
        if n == 1:
            out[name] = int(rec[at]) if name in ("status", "rounds", "K") else rec[at]
        elif name == "H":
            out[name] = [rec[at + i * _CALIB_N: at + i * _CALIB_N + K + 1] for i in range(K + 1)]
        else:
            out[name] = rec[at: at + (K if n == CALIB_MAX_SYSTEMS else K + 1)]
    return out


def _system_scores(scores, what: str) -> Tuple[int, int, int]:
    """(K, P, ld) of scores [K, P] f32 (a 1-D [P] tensor is one system) whose trials are contiguous."""
    if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32 or scores.dim() not in (1, 2):
        raise ValueError(f"{what}: scores is a float32 [K, P] tensor (or [P] for one system)")
    if scores.dim() == 1:
        scores = scores.unsqueeze(0)
    K, P = scores.shape
    if not 1 <= K <= CALIB_MAX_SYSTEMS:
        raise ValueError(f"{what}: K = {K} systems outside [1, {CALIB_MAX_SYSTEMS}]")
    if not 1 <= P < 2 ** 31:
        raise ValueError(f"{what}: P = {P} outside [1, 2^31)")
    ld = _ld(scores)
    if scores.stride(1) != 1 or ld < P:
        raise ValueError(f"{what}: the trials of a system are contiguous and the row stride ld = {ld} >= P = {P}")
    return K, P, ld


def calib_workspace(P: int, device) -> torch.Tensor:
    """The workspace of calib_fit and llr_metrics for P trials."""
    return torch.empty(_workspace_bytes("w2v2_calib_workspace_bytes", P), dtype=torch.uint8, device=device)


llr_metrics_workspace = calib_workspace


def calib_fit(scores, labels, c_miss=1, c_fa=1, p_target=0.05, ridge=0.0, max_iter=32, w_start=None, record=None,
              workspace=None) -> torch.Tensor:
    """Prior-weighted logistic-regression calibration (K = 1) or fusion (K > 1) of scores [K, P] f32 (row stride >= P)
    with labels [P] uint8, both on the device (w2v2_calib_fit) -> the f64 record [CALIB_RECORD_DOUBLES] on the device
    (calib_record_fields names its cells).  The whole fit is enqueued; nothing is copied or waited for.  ``w_start``: K + 1
    host numbers, the first trial point (with ``max_iter=1`` the record then holds J, g and H there)."""
    cost_checks(c_miss, c_fa, p_target, open_prior=True)
    K, P, ld = _system_scores(scores, "calib_fit")
    _labels(labels, P, "calib_fit", "trial")
    if not (isinstance(ridge, (int, float)) and 0 <= ridge < float("inf")):
        raise ValueError(f"calib_fit: ridge = {ridge!r} must be a finite number >= 0")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or not 1 <= max_iter <= 4096:
        raise ValueError(f"calib_fit: max_iter = {max_iter!r} outside [1, 4096]")
    start = None
    if w_start is not None:
        w = [float(v) for v in w_start]
        if len(w) != K + 1 or not all(abs(v) < float("inf") for v in w):
            raise ValueError(f"calib_fit: w_start holds K + 1 = {K + 1} finite numbers")
        start = (C.c_double * (K + 1))(*w)
    record = _out(record, CALIB_RECORD_DOUBLES, scores.device, "calib_fit", "record", torch.float64)
    _dev(scores, labels, record, workspace)
    workspace = _byte_workspace(workspace, _workspace_bytes("w2v2_calib_workspace_bytes", P), scores.device, "calib_fit",
                                "calib_workspace")
    _lib.check(lib().w2v2_calib_fit(scores.data_ptr(), ld, K, labels.data_ptr(), P, float(c_miss), float(c_fa), float(p_target),
                                    float(ridge), max_iter, None if start is None else C.addressof(start), record.data_ptr(),
                                    workspace.data_ptr(), stream()), "calib_fit")
    return record


def calib_apply(scores, record, out=None) -> torch.Tensor:
    """llr [P] f32 = a_0 + sum_k a_k s_k of scores [K, P] (or [P]) with the affine map of a fit's ``record`` -- read on the
    device, no host round trip (w2v2_calib_apply).  ``record``: what calib_fit returned, or a float64 device tensor of
    K + 1 coefficients."""
    K, P, ld = _system_scores(scores, "calib_apply")
    if not isinstance(record, torch.Tensor) or record.dtype != torch.float64 or not record.is_contiguous() \
            or record.numel() not in (K + 1, CALIB_RECORD_DOUBLES):
        raise ValueError(f"calib_apply: record is a fit's float64 record or K + 1 = {K + 1} float64 coefficients")
    out = _out(out, P, scores.device, "calib_apply", "out")
    _dev(scores, record, out)
    a = record if record.numel() == K + 1 else record[CALIB_RECORD["a"][0]:]
    _lib.check(lib().w2v2_calib_apply(scores.data_ptr(), ld, K, P, a.data_ptr(), out.data_ptr(), stream()), "calib_apply")
    return out


def llr_metrics(llr, labels, c_miss=1, c_fa=1, p_target=0.05, out=None, workspace=None) -> torch.Tensor:
    """Cllr and actDCF at the Bayes threshold of llr [P] f32 and labels [P] uint8, both on the device (w2v2_llr_metrics)
    -> out [8] float64 on the device, in the order of LLR_METRICS_FIELDS."""
    cost_checks(c_miss, c_fa, p_target)
    P = _trial_count(llr, torch.float32, "llr_metrics", "llr")
    _labels(labels, P, "llr_metrics", "llr")
    out = _out(out, 8, llr.device, "llr_metrics", "out", torch.float64)
    _dev(llr, labels, out, workspace)
    workspace = _byte_workspace(workspace, _workspace_bytes("w2v2_calib_workspace_bytes", P), llr.device, "llr_metrics",
                                "llr_metrics_workspace")
    _lib.check(lib().w2v2_llr_metrics(llr.data_ptr(), labels.data_ptr(), P, float(c_miss), float(c_fa), float(p_target),
                                      out.data_ptr(), workspace.data_ptr(), stream()), "llr_metrics")
    return out


# ------------------------------------------------------------------------------------------------ waveform augmentation
# (csrc/augment.hip; include/w2v2_hip.h "waveform augmentation" defines every operation.)  Row lists and parameter tables
# are DEVICE tensors the caller built on the host (data/augment.py uploads them in one copy per step): the wrappers check
# shapes and dtypes, which needs no device, and never read a table back.
AUG_MAX_TAPS = 2561                     # W2V2_AUG_MAX_TAPS of include/w2v2_hip.h
AUG_FIR_TILE = 2048                     # outputs per workgroup of w2v2_aug_fir (w2v2_aug_fir_tile())
AUG_RESAMPLE_TILE = 256                 # outputs per workgroup of w2v2_aug_resample (w2v2_aug_resample_tile())
AUG_REVERB_MAX_DELAY = 1024             # W2V2_AUG_REVERB_MAX_DELAY
AUG_REVERB_PARAMS = 28                  # W2V2_AUG_REVERB_PARAMS: int32 per row of w2v2_aug_reverb's table
AUG_REVERB_CHUNK = 512                  # samples per time chunk of w2v2_aug_reverb (w2v2_aug_reverb_chunk())


def _aug_wave(x, what: str) -> Tuple[int, int, int]:
    """(rows, N, ld) of a 2-D float32 waveform buffer whose samples are contiguous."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] < 1 or x.shape[1] < 1 \
            or x.stride(1) != 1:
        raise ValueError(f"{what}: a 2-D float32 [rows, N] tensor with contiguous samples")
    B, N = x.shape
    ld = _ld(x)
    if ld < N:
        raise ValueError(f"{what}: row stride {ld} below N = {N}")
    return B, N, ld


def _aug_i32(t, n: Optional[int], what: str) -> int:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not t.is_contiguous() or (n is not None and t.numel() != n):
        raise ValueError(f"{what}: a contiguous int32 tensor" + (f" of {n} elements" if n is not None else ""))
    return t.numel()


def _aug_rows(rows, what: str) -> int:
    R = _aug_i32(rows, None, f"{what}: rows")
    if rows.dim() != 1 or not 1 <= R <= 65535:
        raise ValueError(f"{what}: rows is an int32 [R] tensor, 1 <= R <= 65535")
    return R


def _aug_lens(lens, B: int, what: str) -> None:
    if lens is not None:
        _aug_i32(lens, B, f"{what}: lens")


def _aug_coef(coef, R: int, what: str) -> None:
    if not isinstance(coef, torch.Tensor) or coef.dtype != torch.float32 or not coef.is_contiguous() or coef.numel() != R:
        raise ValueError(f"{what}: coef is a contiguous float32 [{R}] tensor")


def aug_time_dropout(x, rows, spans, lens=None) -> None:
    """In place: zero the spans[r, s] = (start, length) of row rows[r] of x [B, N], clipped to that row's [0, len)
    (w2v2_aug_time_dropout).  spans: int32 [R, S, 2] on the device (S may be 0); lens: int32 [B] or None."""
    B, N, ld = _aug_wave(x, "aug_time_dropout")
    R = _aug_rows(rows, "aug_time_dropout")
    if not isinstance(spans, torch.Tensor) or spans.dtype != torch.int32 or spans.dim() != 3 or spans.shape[0] != R \
            or spans.shape[2] != 2 or not spans.is_contiguous():
        raise ValueError(f"aug_time_dropout: spans is a contiguous int32 [{R}, S, 2] tensor")
    _aug_lens(lens, B, "aug_time_dropout")
    _dev(x, rows, spans, lens)
    S = spans.shape[1]
    _lib.check(lib().w2v2_aug_time_dropout(x.data_ptr(), ld, N, _p(lens), rows.data_ptr(), R, spans.data_ptr() if S else None, S,
                                           stream()), "aug_time_dropout")


def aug_mix_uniform(x, rows, coef, seed: int, lens=None) -> None:
    """In place: x[row] = coef[r] x[row] + (1 - coef[r]) u, u in [0, 1) from the counter hash keyed by (seed, row number,
    sample index) (w2v2_aug_mix_uniform).  coef: float32 [R] on the device; seed: any Python int, taken modulo 2^64."""
    B, N, ld = _aug_wave(x, "aug_mix_uniform")
    R = _aug_rows(rows, "aug_mix_uniform")
    _aug_coef(coef, R, "aug_mix_uniform")
    _aug_lens(lens, B, "aug_mix_uniform")
    _dev(x, rows, coef, lens)
    s = int(seed) & (2 ** 64 - 1)
    _lib.check(lib().w2v2_aug_mix_uniform(x.data_ptr(), ld, N, _p(lens), rows.data_ptr(), R, coef.data_ptr(),
                                          s - 2 ** 64 if s >= 2 ** 63 else s, stream()), "aug_mix_uniform")


def aug_mix_bank(x, rows, coef, bank, bank_lens, bank_row, lens=None) -> None:
    """In place: the mix of aug_mix_uniform with u = bank[bank_row[r]] repeated to the row's length (w2v2_aug_mix_bank).
    bank: float32 [M, L] on the device, bank_lens: int32 [M], bank_row: int32 [R]."""
    B, N, ld = _aug_wave(x, "aug_mix_bank")
    R = _aug_rows(rows, "aug_mix_bank")
    _aug_coef(coef, R, "aug_mix_bank")
    M, _, ldb = _aug_wave(bank, "aug_mix_bank (bank)")
    _aug_i32(bank_lens, M, "aug_mix_bank: bank_lens")
    _aug_i32(bank_row, R, "aug_mix_bank: bank_row")
    _aug_lens(lens, B, "aug_mix_bank")
    _dev(x, rows, coef, bank, bank_lens, bank_row, lens)
    _lib.check(lib().w2v2_aug_mix_bank(x.data_ptr(), ld, N, _p(lens), rows.data_ptr(), R, coef.data_ptr(), bank.data_ptr(),
                                       ldb, bank_lens.data_ptr(), M, bank_row.data_ptr(), stream()), "aug_mix_bank")


def _aug_src_dst(src, dst, src_rows, dst_rows, lens, what: str):
    Bs, N_in, lds = _aug_wave(src, f"{what} (src)")
    _, N_out, ldd = _aug_wave(dst, f"{what} (dst)")
    R = _aug_rows(src_rows, what)
    if _aug_rows(dst_rows, what) != R:
        raise ValueError(f"{what}: src_rows and dst_rows name {R} rows each")
    _aug_lens(lens, Bs, what)
    if src.untyped_storage().data_ptr() == dst.untyped_storage().data_ptr():
        raise ValueError(f"{what}: src and dst must not share memory")
    return N_in, lds, N_out, ldd, R


def aug_fir(src, dst, src_rows, dst_rows, taps, ntaps, lens=None) -> None:
    """dst[dst_rows[r]] = the zero-phase FIR of src[src_rows[r]] under taps[r, :ntaps[r]] (w2v2_aug_fir): float32 taps
    [R, ldt] and int32 ntaps [R] on the device, every count odd and at most AUG_MAX_TAPS.  lens: int32 per src row."""
    N_in, lds, N_out, ldd, R = _aug_src_dst(src, dst, src_rows, dst_rows, lens, "aug_fir")
    if not isinstance(taps, torch.Tensor) or taps.dtype != torch.float32 or taps.dim() != 2 or taps.shape[0] != R \
            or taps.shape[1] < 1 or taps.stride(1) != 1:
        raise ValueError(f"aug_fir: taps is a float32 [{R}, ldt] tensor")
    _aug_i32(ntaps, R, "aug_fir: ntaps")
    _dev(src, dst, src_rows, dst_rows, taps, ntaps, lens)
    _lib.check(lib().w2v2_aug_fir(src.data_ptr(), lds, N_in, _p(lens), src_rows.data_ptr(), dst.data_ptr(), ldd, N_out,
                                  dst_rows.data_ptr(), R, taps.data_ptr(), _ld(taps), ntaps.data_ptr(), stream()), "aug_fir")


def aug_resample(src, dst, src_rows, dst_rows, U: int, D: int, h=None, lens=None, out_lens=None) -> None:
    """dst[dst_rows[r]] = src[src_rows[r]] resampled by U / D through the prototype h [2 half + 1] (w2v2_aug_resample);
    U == D copies.  out_lens: int32 per dst row, written at the listed rows, or None."""
    N_in, lds, N_out, ldd, R = _aug_src_dst(src, dst, src_rows, dst_rows, lens, "aug_resample")
    if isinstance(U, bool) or isinstance(D, bool) or not isinstance(U, int) or not isinstance(D, int) \
            or not (1 <= U <= 4096 and 1 <= D <= 4096):
        raise ValueError(f"aug_resample: U = {U!r}, D = {D!r}: integers in [1, 4096]")
    half = 0
    if U != D:
        if not isinstance(h, torch.Tensor) or h.dtype != torch.float32 or h.dim() != 1 or not h.is_contiguous() \
                or h.numel() % 2 != 1:
            raise ValueError("aug_resample: h is a contiguous float32 [2 half + 1] tensor")
        half = h.numel() // 2
    if out_lens is not None:
        _aug_i32(out_lens, dst.shape[0], "aug_resample: out_lens")
    _dev(src, dst, src_rows, dst_rows, h if U != D else None, lens, out_lens)
    _lib.check(lib().w2v2_aug_resample(src.data_ptr(), lds, N_in, _p(lens), src_rows.data_ptr(), dst.data_ptr(), ldd, N_out,
                                       dst_rows.data_ptr(), _p(out_lens), R, U, D, h.data_ptr() if U != D else None, half,
                                       stream()), "aug_resample")


def aug_reverb(src, dst, src_rows, dst_rows, params, lens=None) -> None:
    """dst[dst_rows[r]] = the freeverb bank of params[r] over src[src_rows[r]] (w2v2_aug_reverb): int32 params
    [R, AUG_REVERB_PARAMS] on the device -- 16 comb delays, 8 all-pass delays, then the bits of the float32 feedback,
    damp, wet gain and dry gain (data/augment.py reverb_parameters builds a row).  A row with a delay outside
    [1, AUG_REVERB_MAX_DELAY] comes out NaN.  lens: int32 per src row."""
    N_in, lds, N_out, ldd, R = _aug_src_dst(src, dst, src_rows, dst_rows, lens, "aug_reverb")
    if not isinstance(params, torch.Tensor) or params.dtype != torch.int32 or params.dim() != 2 \
            or tuple(params.shape) != (R, AUG_REVERB_PARAMS) or not params.is_contiguous():
        raise ValueError(f"aug_reverb: params is a contiguous int32 [{R}, {AUG_REVERB_PARAMS}] tensor")
    _dev(src, dst, src_rows, dst_rows, params, lens)
    _lib.check(lib().w2v2_aug_reverb(src.data_ptr(), lds, N_in, _p(lens), src_rows.data_ptr(), dst.data_ptr(), ldd, N_out,
                                     dst_rows.data_ptr(), R, params.data_ptr(), stream()), "aug_reverb")
