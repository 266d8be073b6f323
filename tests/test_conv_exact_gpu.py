"""Every convolution kernel path against a float64 reference, element for element.

Integer-valued bf16 operands make every output exactly representable and every fp32 partial sum an
integer below 2^24 (serverless_learn_amd/utils/conv_exact.py), so each case asserts ``torch.equal``
on every output -- forward y / yf / statistics, data gradient with and without the residual add
(and the even-position shortcut forms), weight gradient by atomics and by slab for three split-K
targets -- and that the kernel family the case is in the table for is the one that ran.  A single
wrong element, which the norm-wise bounds of test_cnn_gpu.py cannot see (tests/test_conv_exact.py),
fails here, and the message says where it is."""
import json
import os
import subprocess
import sys

import pytest
import torch

from serverless_learn_amd.utils import conv_exact as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_conv_exact(case):
    r = X.run_case(case)
    print(json.dumps(r))
    assert not r["failures"], "\n".join(r["failures"])


@pytest.mark.parametrize("case", [c for c in X.CASES if c.group == "G"], ids=lambda c: c.name)
def test_direct_3x3_equals_implicit_gemm_bit_for_bit(case):
    """The direct kernels' outputs and the same case with the direct path switched off."""
    a = X.run_case(case, keep=True)
    b = X.run_case(X.gemm_twin(case), keep=True)
    assert not a["failures"] and not b["failures"], "\n".join(a["failures"] + b["failures"])
    assert any(f.startswith("halo") for f in a["seen"]["fwd"]), a["seen"]
    assert not any(f.startswith("halo") for fams in b["seen"].values() for f in fams), b["seen"]
    for key in ("y", "dx_add", "dw"):
        assert torch.equal(a["out"][key], b["out"][key]), key


def test_data_gradient_refuses_a_source_stride_that_is_no_power_of_two():
    """The guard case A3 works around (docs/CONV_EXACT.md): dY with 72 channels per pixel is
    refused by the data-gradient launcher before anything is launched, not served wrongly."""
    from serverless_learn_amd.ops import cnn as K

    dy = torch.zeros(1, 6, 10, 72, dtype=torch.bfloat16, device="cuda")
    wt = torch.zeros(64 * 72, dtype=torch.bfloat16, device="cuda")
    dx = torch.full((1, 6, 10, 64), 7.0, dtype=torch.bfloat16, device="cuda")
    K.conv_kernels_seen(clear=True)
    with pytest.raises(RuntimeError, match="code -1"):
        K.conv_dgrad(dy, wt, 64, 1, 1, 0, dx)
    torch.cuda.synchronize()
    assert not K.conv_kernels_seen() and bool((dx == 7.0).all())


def _child(subset, env):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "conv_exact_check.py"), subset],
                         env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(r))
    assert [c["name"] for c in r["cases"]] == X.SUBSETS[subset], r
    bad = [(c["name"], c["failures"]) for c in r["cases"] if c["failures"]]
    assert not bad, bad
    return r


def test_conv_exact_deterministic_build():
    """SL_DETERMINISTIC=1 (own process): the 2^8 / 2^40 fixed-point cross-workgroup sums and the
    slab-only split-K are exact on integers -- statistics and dW included -- for one case each of
    the big, wide, stride-2, weight-gradient and direct kernels."""
    r = _child("det", dict(os.environ, SL_DETERMINISTIC="1"))
    assert r["deterministic_build"] and not r["smallm"], r


def test_conv_exact_forced_128_row_tiles():
    """SL_GEMM_SMALLM=1 (own process): the small-tile cases through the 128-row conv_gemm_kernel
    instantiations, forward and transposed, at small M with row tails."""
    env = {k: v for k, v in os.environ.items() if k != "SL_DETERMINISTIC"}
    r = _child("smallm", dict(env, SL_GEMM_SMALLM="1"))
    assert r["smallm"] and not r["deterministic_build"], r
    seen = {f for c in r["cases"] for fams in c["seen"].values() for f in fams}
    assert {"gemm_128x64", "gemm_128x128", "gemm_t_128x64", "gemm_t_128x128"} <= seen, seen
