#!/usr/bin/env python3
"""Exact MLP cases (serverless_learn_amd/utils/mlp_exact.py) in a fresh process: a process loads one
kernel library and reads SL_DETERMINISTIC once, so the deterministic build needs its own.  Runs a
named subset of the case table -- "det" (S64, S128, S320) -- "all", or the cases named on the
command line: each with the tiled and the row-major shard, then the three update forms of those
that are update cases.  Prints one JSON line: per run the mismatches found (none = every buffer
equals the float64 reference), the rows tile / slices / X layout that ran, the reference maxima and
the worst loss deviation relative to its bound.
Usage: [SL_DETERMINISTIC=1] python scripts/mlp_exact_check.py det|all|CASE..."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from serverless_learn_amd.ops import cnn as K
from serverless_learn_amd.utils import mlp_exact as X

args = sys.argv[1:] or ["det"]
if args == ["all"]:
    names = [c.name for c in X.CASES]
elif len(args) == 1 and args[0] in X.SUBSETS:
    names = X.SUBSETS[args[0]]
else:
    names = args
cases = [X.run_case(X.CASES_BY_NAME[n], xt=xt) for n in names for xt in (True, False)]
updates = [X.run_update(X.CASES_BY_NAME[n]) for n in names if X.CASES_BY_NAME[n].update]
print(json.dumps({"deterministic_build": K.deterministic(), "cases": cases, "updates": updates}))
