"""CPU side of the GEMM edge cases (tests/gemm_cases.py): ties the case table to its references and bounds without a GPU.

* every case's operands meet the exact-class conditions (``problem`` asserts them while it builds) and a plain f32
  implementation -- torch's own CPU f32 matmul with f32 epilogue arithmetic -- passes ``judge``: the exact class bit for
  bit, the real class inside the derived bound, so the bound is one the reference passes;
* the f32 restatement of the erf polynomial stays inside the GELU bound on a 1/256 grid of [-8, 8];
* ``judge`` does notice what it is there for: one wrong element, one NaN left, one guard cell written;
* every case's descriptor is routed to the family it names by ``w2v2_gemm_kernel_of`` at the 256-CU fallback, in a
  fresh process per tuner setting (like test_host_cpu.py::test_gemm_routing_table)."""
import collections
import json
import os
import subprocess
import sys

import pytest
import torch

import gemm_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CUS = 8          # the persistent-round shapes follow the CU count; their conditions do not depend on M


def test_case_table_covers_every_family_and_names_are_unique():
    cases = GC.all_cases(256)
    assert len({cs["name"] for cs in cases}) == len(cases) > 6000
    fams = collections.Counter(cs["fam"] for cs in cases)
    assert set(fams) == {1, 2, 3, 4, 9, 10} and min(fams.values()) >= 150
    for cs in cases:
        lay = GC.layout(cs)
        assert lay["ldc"] >= cs["N"] + 8 and lay["ldaux"] >= lay["ldc"]
    # the persistent rounds: more tiles than CUs, fewer than two rounds, a ragged last M tile
    for fam, bn in ((2, 128), (4, 256)):
        for n in (256, 304, 64):
            M, N = GC.round_shape(fam, n)
            tiles = -(-M // 256) * (N // bn)
            assert n + 5 <= tiles < 2 * n and M % 256 == 256 - 37
    # family 1 with 128 x 128 tiles: more than half of the CUs get a tile (gemm_route's test for the 64-column tile)
    for n in (256, 304, 64):
        M, N = GC.wide_shape(n)
        assert -(-M // 128) * (N // 128) * 2 > n and -(-M // 128) * -(-(N - 56) // 128) * 2 > n and M % 128 == 128 - 37
    assert all(-(-cs["M"] // 128) * -(-cs["N"] // 128) * 2 > 256 for cs in cases if cs["group"] == "wide")
    # every descriptor feature on every 16-bit family and on family 10
    feats = {(e, cls, tuple(sorted(kw.items()))) for (e, cls, kw) in GC.feature_options()}
    for fam in (1, 2, 3, 4, 10):
        for ab in (("f32",) if fam == 10 else GC.LP):
            for c in {ab, "f32"}:
                mine = [cs for cs in cases if cs["group"] == "feature" and cs["fam"] == fam and cs["ab"] == ab and cs["c"] == c]
                got = {(cs["epi"], cs["cls"], tuple(sorted((k, cs[k]) for k in GC.DEFAULTS
                                                           if cs[k] != GC.DEFAULTS[k] and k not in ("tune", "ta", "tb"))))
                       for cs in mine}
                # (a 16-bit C with its aux one element off has no whole lines: the phased kernel hands it to the ring)
                want = feats if fam != 4 or c == "f32" else {f for f in feats if dict(f[2]).get("aux_off", 0) == 0}
                assert want <= got, (fam, ab, c, sorted(want - got)[:3])
                if c == "f32" and fam in (1, 3, 10):             # accumulate and split-K need an f32 C
                    assert {cs["cls"] for cs in mine if cs["accumulate"]} == {"exact", "real"}
                    assert {cs["split"] for cs in mine} == {1, 2, 3, 5}
    assert {cs["fam"] for cs in cases if cs["accumulate"]} == {1, 3, 10}     # (atomics leave the ring and the phased kernel)
    assert {(cs["ta"], cs["tb"]) for cs in cases if cs["group"] == "feature" and cs["fam"] == 3} >= {(False, False), (True, False), (False, True)}
    # deferred stores with three and four K steps need a 16-bit C, N % 128 == 0, no GELU kind: all in the round cases
    defer = [cs for cs in cases if cs["group"] == "rounds" and cs["fam"] == 2 and cs["c"] != "f32"]
    assert {cs["K"] for cs in defer} == {64, 192, 256, 320} and {cs["epi"] for cs in defer} == {"none", "add", "bias"}
    assert all(GC.lines_rule(cs, GC.layout(cs)) and cs["N"] % 128 == 0 for cs in defer)


@pytest.mark.parametrize("group", ["sweep", "epilogue", "feature", "regstage", "rounds", "conv", "batched", "two_term", "wide", "f32"])
def test_cases_meet_their_conditions_and_an_f32_reference_passes(group):
    seen, worst = set(), collections.defaultdict(float)
    for cs in GC.all_cases(SMALL_CUS):
        key = GC._operand_key(cs)
        if cs["group"] != group or key in seen:
            continue
        seen.add(key)
        p = GC.problem(cs)                                      # asserts the exact-class conditions
        r = GC.judge(cs, p, *GC.emulate_f32(cs, p))             # asserts the element checks and the guards
        worst[(cs["c"], cs["cls"])] = max(worst[(cs["c"], cs["cls"])], r["ratio"])
        if cs["cls"] == "gelu":
            assert max(p["gelu_E"]) < 1e-6                      # (torch's f32 gelu: 2.5e-7 when this was written)
    assert seen
    for (c, cls), w in sorted(worst.items()):
        print(f"gemm-parity: cpu f32 reference, {group}, C {c}, {cls}: max error / bound {w:.3f} over the group")
        assert w <= 1.0 and (cls != "exact" or w == 0.0)


def test_erf_polynomial_in_f32_stays_inside_the_gelu_bound():
    x = (torch.arange(-8 * 256, 8 * 256 + 1, dtype=torch.float64) / 256)
    x32 = x.float()
    mx = x.abs().clamp_min(1.0)
    for deriv, poly, ref in ((False, GC.gelu_poly_f32, GC.gelu64), (True, GC.dgelu_poly_f32, GC.dgelu64)):
        E = GC.gelu_E(x, deriv)
        err = (poly(x32).double() - ref(x)).abs() / mx
        bound = GC.GELU_POLY_HALF + 2 * E
        print(f"gemm-parity: cpu erf polynomial in f32, {'gelu_grad' if deriv else 'gelu'}: E {E:.3e}, max error / max(1, |x|) "
              f"{float(err.max()):.3e}, bound {bound:.3e}")
        assert float(err.max()) <= bound


def test_judge_notices_one_wrong_element_a_nan_and_a_written_guard_cell():
    for cs in (GC.forced("sweep", 2, 257, 192, 192, "bf16", "bf16", "exact"), GC.forced("sweep", 2, 257, 192, 192, "f16", "f32", "real"),
               GC.forced("epilogue", 1, 257, 100, 128, "f16", "f16", "gelu", "bias_gelu", alpha=2.0 ** -5)):
        p = GC.problem(cs)
        c, aux = GC.emulate_f32(cs, p)
        GC.judge(cs, p, c, aux)
        lay = p["lay"]
        at = int(p["c_idx"][0, 0, cs["M"] - 1, cs["N"] - 1])
        for mutate in ("value", "nan", "guard_col", "guard_row", "chunk"):
            c2 = c.clone()
            if mutate == "value":                                # one element off by 1/64 of max(1, its size) (exact class: by one)
                c2[at] = c2[at] + 2.0 ** -6 * max(1.0, abs(float(c2[at]))) if cs["cls"] != "exact" else c2[at] + 1
                assert c2[at] != c[at]
            elif mutate == "nan":
                c2[at] = float("nan")
            elif mutate == "guard_col":
                c2[at + 1] = 0.0
            elif mutate == "guard_row":
                c2[int(p["c_idx"][0, 0, 0, 0]) - lay["ldc"]] = 0.0
            else:                                                # one 8-wide K chunk dropped from one element
                if cs["cls"] != "real":
                    continue
                m, n = 100, 37
                full = p["A"][0, 0, m] @ p["B"][0, n]
                c2[int(p["c_idx"][0, 0, m, n])] = float(full - p["A"][0, 0, m, 64:72] @ p["B"][0, n, 64:72])
            with pytest.raises(AssertionError):
                GC.judge(cs, p, c2, aux)
        if aux is not None:
            a2 = aux.clone()
            a2[int(p["aux_idx"][0, 0, 3, 5])] += 1
            with pytest.raises(AssertionError):
                GC.judge(cs, p, c, a2)


def test_every_case_is_routed_to_the_family_it_names():
    cases = GC.all_cases(256)
    settings = GC.tune_settings(cases)
    assert settings == sorted([""] + [f"kernel={k}" for k in (1, 2, 4)] + [f"f32_tile={t}" for t in (0,) + GC.F32_CODES])
    env = {k: v for k, v in os.environ.items() if k not in GC.SWITCHES and k != "W2V2_LIB_AB"}
    procs = [(s, subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "gemm_cases.py")], env=dict(env, ROUTE_TUNE=s),
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for s in settings]
    total = 0
    for s, pr in procs:
        out, err = pr.communicate(timeout=600)
        line = [l for l in out.splitlines() if l.startswith("ROUTE ")]
        assert line, (s, err[-2000:])
        rows = json.loads(line[0][6:])
        assert len(rows) == sum(GC.tune_name(cs) == s for cs in cases) > 0
        wrong = [r for r in rows if r[1] != r[2]]
        assert not wrong, (s, len(wrong), wrong[:5])
        total += len(rows)
    assert total == len(cases)
