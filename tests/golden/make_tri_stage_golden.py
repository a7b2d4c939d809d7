#!/usr/bin/env python3
"""Generate tests/golden/tri_stage.json by RUNNING THE REFERENCE's tri-stage schedule class (authoring container only).

Imports /root/reference/src/optim/schedule/tri_stage.py (read-only, CPU) and records the factor it returns at every
step 0 .. max_steps + 2 for a handful of configurations.  A step at which the reference raises (its decay table is
two points longer than floor(max_steps * ratio); where the three floors lose two or more steps the last steps index
past it) is recorded as null with the exception's class name under "raises".  Data only; no reference source travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_tri_stage_golden.py
"""
import importlib.util
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src/optim/schedule/tri_stage.py"

spec = importlib.util.spec_from_file_location("ref_tri_stage", REF)
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)

LRS = dict(initial_lr=1e-7, base_lr=1e-4, final_lr=1e-8)
CASES = [dict(max_steps=m, warmup_stage_ratio=0.1, constant_stage_ratio=0.4, decay_stage_ratio=0.5, **LRS)
         for m in (10, 37, 1000)]
CASES.append(dict(max_steps=100, warmup_stage_ratio=0.0, constant_stage_ratio=0.5, decay_stage_ratio=0.5, **LRS))

out = []
for kw in CASES:
    fn = mod.TriStageLearningRateLambdaLRFunction(**kw)
    factors, raises = [], {}
    for step in range(kw["max_steps"] + 3):
        try:
            factors.append(float(fn(step)))
        except Exception as e:          # recorded, not hidden: the port must raise the same class at the same step
            factors.append(None)
            raises[str(step)] = type(e).__name__
    out.append({"config": kw, "factors": factors, "raises": raises})
with open(os.path.join(HERE, "tri_stage.json"), "w") as f:
    json.dump(out, f, indent=0)
print("wrote tri_stage.json:", [(c["config"]["max_steps"], c["raises"]) for c in out])
