#!/usr/bin/env python3
"""Generate tests/golden/g20_paired_varlen.npz by RUNNING THE REFERENCE's modules (authoring container only).

The paired-input model at UNEQUAL lengths (ref: src/lightning_modules/speaker/wav2vec2_paired_input.py:163-207 with the
contract of paired_speaker_recognition_module.py:51-60: [BATCH, N] and [BATCH, M]).  Uses make_goldens' shims and
``build_reference_wrapper`` (tiny config, weights seed 20211, evaluation mode); each pair goes ALONE through the wrapper's
own ``feature_extractor``, ``feature_projection`` and ``encoder``, concatenated as lines :171-205 do, with CLS = 1 and
SEP = -1 (the module config's defaults).

Deviation, on purpose: the reference builds its three tokens 768 wide (:183-193), which only fits wav2vec2-base; here the
token width is the configuration's ``hidden_size`` (64 for the tiny config), everything else is as the reference does it.
The fixture is data only; no reference source travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_paired_goldens.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_goldens as MG  # noqa: E402  (shims, reference imports, build_reference_wrapper)
from make_goldens import O  # noqa: E402

LEFT = [4000, 400, 2500, 26000]
RIGHT = [400, 4000, 3217, 26000]
CLS, SEP = 1.0, -1.0


def golden_paired_varlen():
    cfg = O.OracleConfig.tiny()
    w, _ = MG.build_reference_wrapper(cfg, 20211)
    w.eval()
    model = w.model
    wl, _ = O.synth_batch(4, 26000, 2, seed=21)
    wr, _ = O.synth_batch(4, 26000, 2, seed=22)
    H = cfg.hidden_size
    token0, full2 = [], None
    with torch.no_grad():
        for b, (na, nb) in enumerate(zip(LEFT, RIGHT)):
            a, c = wl[b:b + 1, 0, :na], wr[b:b + 1, 0, :nb]
            f1 = model.feature_extractor(a).transpose(1, 2)
            f2 = model.feature_extractor(c).transpose(1, 2)
            f1, _ = model.feature_projection(f1)
            f2, _ = model.feature_projection(f2)
            tok = lambda v: torch.ones((1, 1, H)) * v
            seq = torch.cat([tok(CLS), f1, tok(SEP), f2, tok(SEP)], dim=1)
            out = model.encoder(seq).last_hidden_state
            assert out.shape[1] == f1.shape[1] + f2.shape[1] + 3
            token0.append(out[0, 0])
            if b == 2:
                full2 = out[0]
    g = {"left_lengths": np.asarray(LEFT, dtype=np.int64), "right_lengths": np.asarray(RIGHT, dtype=np.int64),
         "token0": torch.stack(token0), "pair2.last_hidden_state": full2}
    np.savez_compressed(os.path.join(MG.OUT, "g20_paired_varlen.npz"), **MG.to_np(g))
    print("g20_paired_varlen: frames", [int(x) for x in (full2.shape[0],)], "token0 norm",
          [round(float(t.norm()), 4) for t in token0])


if __name__ == "__main__":
    golden_paired_varlen()
