"""Float64 statements of the tap gather and its adjoint (csrc/tap_gather.h) for tests/test_tap_gather_gpu.py, written as
plain index loops over the index map p(t, j) = t * stride + j * dil - pad, and the integer-valued inputs of those tests.

Every input is an integer in [-8, 8].  A gathered element is one of them or the sum of two; an element of the adjoint is a
sum of at most 3 k of them (k taps, at most three images per tap under reflect padding) plus, when it accumulates, one
prior value: at most 3 * 5 * 8 + 8 = 128 in magnitude with the k <= 5 used here, (10 * 8 = 80 for the k = 10 zero case),
and every partial sum is an integer no larger.  Integers up to 256 are exact in bf16, up to 2048 in f16, up to 2^24 in f32,
so every order of addition gives the same bits and the device must equal the float64 result exactly."""
import torch

F64 = torch.float64


def ints(shape, seed: int) -> torch.Tensor:
    """Integer-valued float64 in [-8, 8]."""
    return torch.randint(-8, 9, tuple(shape), generator=torch.Generator().manual_seed(seed)).to(F64)


def frames_of(Tin: int, k: int, stride: int, pad: int) -> int:
    return (Tin + 2 * pad - k) // stride + 1


def reflect(p: int, L: int) -> int:
    if p < 0:
        p = -p
    if p >= L:
        p = 2 * (L - 1) - p
    return p


def source_row(p: int, L: int, mode: str):
    """The row position p reads, or None."""
    if mode == "reflect":
        return reflect(p, L)
    return p if 0 <= p < L else None


def gather_ref(x_btc: torch.Tensor, Tout: int, k: int, stride: int, dil: int, pad: int, mode: str) -> torch.Tensor:
    """[B, Tin, C] -> [B * Tout, k * C] float64; positions that read nothing are +0.0."""
    B, Tin, C = x_btc.shape
    col = torch.zeros(B, Tout, k, C, dtype=F64)
    for t in range(Tout):
        for j in range(k):
            s = source_row(t * stride + j * dil - pad, Tin, mode)
            if s is not None:
                col[:, t, j] = x_btc[:, s].to(F64)
    return col.reshape(B * Tout, k * C)


def adjoint_ref(dcol: torch.Tensor, B: int, Tin: int, Tout: int, C: int, k: int, stride: int, dil: int, pad: int,
                mode: str) -> torch.Tensor:
    """[B * Tout, k * C] -> [B, Tin, C] float64: the scatter-add that is the transpose of gather_ref (rows no frame
    reaches stay zero)."""
    d = dcol.to(F64).reshape(B, Tout, k, C)
    dx = torch.zeros(B, Tin, C, dtype=F64)
    for t in range(Tout):
        for j in range(k):
            s = source_row(t * stride + j * dil - pad, Tin, mode)
            if s is not None:
                dx[:, s] += d[:, t, j]
    return dx
