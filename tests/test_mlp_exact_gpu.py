"""Every buffer of the fused MLP step against a float64 reference, element for element.

Power-of-two launch scalars and integer-valued operands make every quantity of the step exactly
representable where the kernels store it (serverless_learn_amd/utils/mlp_exact.py), so each case
asserts ``torch.equal`` on H1, dH2, dH1, ``correct``, every partial row of [dW3 | db3 | db1 | db2],
the evaluation form's logits, the reduced gradient of every parameter tensor and -- from a preset
momentum, through each of the three update forms -- parameters, momentum, the five decoded shadows
and the W1 row totals; the per-row loss keeps the bound derived for its logarithm.  Each case also
asserts the rows tile, the split-K slice count and the X layout it is in the table for.  A single
wrong element, which the norm-wise bounds of test_mlp_fused_gpu.py cannot see or cannot place
(tests/test_mlp_exact.py), fails here, and the message says where it is."""
import json
import os
import subprocess
import sys

import pytest

from serverless_learn_amd.utils import mlp_exact as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("layout", ["xt", "rowmajor"])
@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_mlp_exact(case, layout):
    r = X.run_case(case, xt=layout == "xt")
    print(json.dumps(r))
    assert not r["failures"], "\n".join(r["failures"])
    assert [(v["bm"], v["slices"], v["xt"]) for v in r["ran"]] == [(case.bm, s, layout == "xt") for _, s in case.slices]


@pytest.mark.parametrize("case", X.UPDATE_CASES, ids=lambda c: c.name)
def test_mlp_update_exact(case):
    r = X.run_update(case)
    print(json.dumps(r))
    assert not r["failures"], "\n".join(r["failures"])
    assert len(r["ran"]) == len(X.UPDATE_FORMS)


def test_mlp_exact_deterministic_build():
    """SL_DETERMINISTIC=1 (own process: a process loads one kernel library): S64, S128 and S320, both
    X layouts, and the update of the first two."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "mlp_exact_check.py"), "det"],
                         env=dict(os.environ, SL_DETERMINISTIC="1"), capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(r))
    assert r["deterministic_build"], r
    assert [c["name"] for c in r["cases"]] == [n for n in X.SUBSETS["det"] for _ in range(2)], r
    assert [c["name"] for c in r["updates"]] == [n for n in X.SUBSETS["det"] if X.CASES_BY_NAME[n].update], r
    bad = [(c["name"], c["failures"]) for c in r["cases"] + r["updates"] if c["failures"]]
    assert not bad, bad
