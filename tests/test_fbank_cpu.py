"""Device log-mel front-end of the ECAPA path, host side: the frame count, the validation of
EcapaPlan.embed_waveform(lengths=), the module's ``input_features`` keyword and the two new C-ABI symbols (no GPU
needed)."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["w2v2_fbank_db", "w2v2_fbank_normalize"]


def test_fbank_frames_is_the_host_front_ends_frame_count():
    from w2v2_speaker_amd.data.fbank import Fbank
    from w2v2_speaker_amd.ecapa import fbank_frames
    want = {159: 1, 160: 2, 161: 2, 640: 5, 48000: 301}
    for n, frames in want.items():
        assert fbank_frames(n) == frames == 1 + n // 160, n
    fb = Fbank()
    for n in (640, 48000):            # (torch.stft refuses inputs shorter than its centre padding allows: 159..161 by rule)
        assert fb(torch.zeros(n)).shape[0] == fbank_frames(n)


def test_sample_length_validation():
    from w2v2_speaker_amd.ecapa import EcapaConfig, ecapa_min_frames, fbank_frames, valid_sample_lengths
    cfg = EcapaConfig()
    lo = 160 * (ecapa_min_frames(cfg) - 1)
    assert lo == 640 and fbank_frames(lo) == ecapa_min_frames(cfg) and fbank_frames(lo - 1) == ecapa_min_frames(cfg) - 1
    assert valid_sample_lengths(cfg, [48000, 640], 2, 48000) == [48000, 640]
    assert valid_sample_lengths(cfg, torch.tensor([48000, 801]), 2, 48000) == [48000, 801]
    assert valid_sample_lengths(cfg, torch.tensor([[700], [900]], dtype=torch.int32), 2, 1000) == [700, 900]
    with pytest.raises(ValueError):
        valid_sample_lengths(cfg, [48001, 640], 2, 48000)         # longer than the batch
    with pytest.raises(ValueError):
        valid_sample_lengths(cfg, [48000, 639], 2, 48000)         # four frames: shorter than the reflect padding allows
    with pytest.raises(ValueError):
        valid_sample_lengths(cfg, [48000], 2, 48000)              # one per row
    with pytest.raises(ValueError):
        valid_sample_lengths(cfg, [48000, 640, 640], 2, 48000)
    with pytest.raises(ValueError):
        valid_sample_lengths(cfg, torch.tensor([48000.0, 640.0]), 2, 48000)
    if torch.cuda.is_available():
        with pytest.raises(ValueError):
            valid_sample_lengths(cfg, torch.tensor([48000, 640], device="cuda"), 2, 48000)
    # a model with a wider reflect padding needs more samples
    wide = EcapaConfig(kernel_sizes=(5, 3, 3, 3, 1), dilations=(4, 2, 3, 4, 1))
    assert valid_sample_lengths(wide, [1280], 1, 1280) == [1280]
    with pytest.raises(ValueError):
        valid_sample_lengths(wide, [1279], 1, 1280)


def _c_params(hdr: str, name: str):
    """ctypes-level kinds of the parameters of ``int name(...)`` in the header: 'p' pointer, 'i64', 'i32', 'f32'."""
    m = re.search(r"\bint " + name + r"\(([^;]*?)\);", hdr, re.S)
    assert m, name
    kinds = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        if "*" in p:
            kinds.append("p")
        elif p.startswith("int64_t "):
            kinds.append("i64")
        elif p.startswith("int "):
            kinds.append("i32")
        elif p.startswith("float "):
            kinds.append("f32")
        else:
            raise AssertionError(f"{name}: parameter {p!r}")
    return kinds


def test_new_symbols_declared_exported_and_wrapped_with_matching_signatures():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    from w2v2_speaker_amd import _build, _lib, ops
    kind = {C.c_void_p: "p", C.c_int64: "i64", C.c_int32: "i32", C.c_float: "f32"}
    for name in NEW_SYMBOLS:
        assert name in _lib._SIGS and name in _lib.EXPORTS, name
        res, args = _lib._SIGS[name]
        assert res is C.c_int32
        assert [kind[a] for a in args] == _c_params(hdr, name), name
    # the parser itself, on an entry that has been there all along
    assert [kind[a] for a in _lib._SIGS["w2v2_pool_fwd_len"][1]] == _c_params(hdr, "w2v2_pool_fwd_len")
    assert "fbank.hip" in _build.SOURCES
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    for fn in ("fbank_db", "fbank_normalize", "fbank_partial_max"):
        assert callable(getattr(ops, fn)), fn
    assert f"#define W2V2_FBANK_TILE_FRAMES {ops.FBANK_TILE_FRAMES}\n" in hdr
    assert (ops.FBANK_HOP, ops.FBANK_WIN) == (160, 400)


def test_device_front_end_constants_are_the_host_front_ends():
    from w2v2_speaker_amd import ops
    from w2v2_speaker_amd.data.fbank import Fbank
    fb = Fbank()
    assert (fb.n_fft, fb.win, fb.hop) == (ops.FBANK_WIN, ops.FBANK_WIN, ops.FBANK_HOP)
    assert tuple(fb.fbank.shape) == (ops.FBANK_WIN // 2 + 1, 40)
    assert torch.equal(fb.window, torch.hamming_window(400))


def test_module_and_plan_surface():
    from w2v2_speaker_amd.ecapa import EcapaPlan
    from w2v2_speaker_amd.lightning_modules.speaker.ecapa_tdnn import EcapaTdnnModule
    p = inspect.signature(EcapaTdnnModule.__init__).parameters["input_features"]
    assert p.default == "fbank" and p.kind is inspect.Parameter.KEYWORD_ONLY
    q = inspect.signature(EcapaPlan.embed_waveform).parameters
    assert list(q) == ["self", "wav", "lengths"] and q["lengths"].default is None
