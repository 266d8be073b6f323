#!/usr/bin/env python3
"""Exact convolution cases (serverless_learn_amd/utils/conv_exact.py) in a fresh process: a process
loads one kernel library and reads the SL_* knobs once, so the deterministic build and the forced
128-row tiles each need their own.  Runs a named subset of the case table -- "det" (one case each
of the large-tile, stride-2, weight-gradient and direct kernels) or "smallm" (the small-tile
cases) -- or the cases named on the command line, and prints one JSON line: per case the
mismatches found (none = every output equals the float64 reference), the kernel families launched,
the density and the reference maxima.
Usage: [SL_DETERMINISTIC=1 | SL_GEMM_SMALLM=1] python scripts/conv_exact_check.py det|smallm|all|CASE..."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from serverless_learn_amd.ops import cnn as K
from serverless_learn_amd.utils import conv_exact as X

args = sys.argv[1:] or ["det"]
if args == ["all"]:
    names = [c.name for c in X.CASES]
elif len(args) == 1 and args[0] in X.SUBSETS:
    names = X.SUBSETS[args[0]]
else:
    names = args
smallm = os.environ.get("SL_GEMM_SMALLM") == "1"
cases = [X.run_case(X.CASES_BY_NAME[n], "cuda:0", smallm=smallm) for n in names]
print(json.dumps({"deterministic_build": K.deterministic(), "smallm": smallm, "cases": cases}))
