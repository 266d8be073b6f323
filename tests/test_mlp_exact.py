"""The exact-MLP checker checked on the CPU (serverless_learn_amd/utils/mlp_exact.py): the conditions
that make every buffer of the step exactly representable, its float64 reference against float64
autograd of the same model, its comparator's messages, and a record of five localized faults: what
the norm-wise bounds of tests/test_mlp_fused_gpu.py say to each, and that the exact comparison
rejects and locates every one.  That record is why tests/test_mlp_exact_gpu.py exists."""
import functools

import pytest
import torch
import torch.nn.functional as F

from serverless_learn_amd.data.synthetic import make_mnist_like
from serverless_learn_amd.models import mlp as M
from serverless_learn_amd.utils import mlp_exact as X


def test_case_table_is_consistent():
    names = [c.name for c in X.CASES]
    assert names == ["S64", "S128", "S128h", "S320", "S384", "S1792", "C256", "P128", "T128"]
    assert [c.name for c in X.UPDATE_CASES] == ["S64", "S128", "S384"] and X.SUBSETS["det"] == ["S64", "S128", "S320"]
    for c in X.CASES:
        assert c.batch % 64 == 0 and c.rows % c.batch == 0 and c.batch % c.bm == 0 and c.why, c.name
        assert c.grad_scale == 2.0 ** -round(torch.log2(torch.tensor(float(c.batch))).item()), c.name
        assert c.grad_scale * c.dh1_scale == 2.0 ** -7
        # the slice arithmetic of sl_mlp_wgrad_slices: whole 64-row stages, equal slices but the last
        for req, want in c.slices:
            total = c.batch // 64
            r = min(req or 28, total)
            spp = -(-total // r)
            assert -(-total // spp) == want, (c.name, req, want)
    by = X.CASES_BY_NAME
    assert by["S320"].slices == ((3, 3),) and 320 // 64 == 2 + 2 + 1
    assert by["S384"].slices == ((4, 3), (None, 6)) and by["S1792"].slices == ((None, 28),)
    assert by["S128h"].force_bm == 64 and by["S128h"].bm == 64 and by["S128"].bm == 128
    assert by["C256"].rows == 256 and by["C256"].cursor == 1
    assert (by["P128"].xa, by["P128"].xb) == (2.0 ** -6, -1.0) and (by["S64"].xa, by["S64"].xb) == (1.0, -1.0)


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_bounds_hold(case):
    """Every condition of check_case_bounds on the reference alone, with margin where a margin
    means something: the GEMM sums at most a quarter of 2^24."""
    ref = X.reference(case)
    s = X.check_case_bounds(case, ref)
    assert max(ref["sumabs"].values()) < 2 ** 23, ref["sumabs"]
    assert ref["maxima"]["h1"] <= 128 and ref["maxima"]["h2"] <= 256, ref["maxima"]
    assert s["p2_zero"] > 0, s  # exact zeros at layer 2 as well
    o = X.operands(case)
    x = o["x"].double() / case.x_step
    assert torch.equal(x, x.round()) and float(x.max()) == 3.0 and abs(float((x != 0).double().mean()) - 0.125) < 0.01
    if case.name == "C256":  # batch 0 holds other pixels than the batch the cursor selects
        assert not torch.equal(o["x"][:128], o["x"][128:])
        assert torch.equal(ref["xu"], o["x"][128:].double())


def test_table_bounds_hold():
    X.check_table_bounds({c.name: X.reference(c) for c in X.CASES})


def test_operands_are_seeded():
    case = X.CASES_BY_NAME["S64"]
    a = X.operands(case)
    X.operands.cache_clear()
    b = X.operands(case)
    assert all(torch.equal(a[k], b[k]) for k in ("x", "y", "flat", "mom0"))
    assert not torch.equal(a["flat"], X.operands(X.CASES_BY_NAME["S128"])["flat"])


@pytest.mark.parametrize("case", [c for c in X.CASES if c.batch <= 384], ids=lambda c: c.name)
def test_reference_matches_float64_autograd(case):
    """Forward, per-row loss and every gradient of the reference against float64 torch autograd of
    the same model with the case's xa / xb, then torch's own SGD.  Not exact: float64 exp(-128) is
    not 0, so autograd's probabilities differ from 1/m by ~1e-56."""
    o, ref = X.operands(case), X.reference(case)
    flat = o["flat"].double().clone().requires_grad_(True)
    v = M.views(flat)
    xn = ref["xu"] * case.xa + case.xb
    h = F.relu(F.linear(xn, v["fc1.weight"], v["fc1.bias"]))
    h = F.relu(F.linear(h, v["fc2.weight"], v["fc2.bias"]))
    z = F.linear(h, v["fc3.weight"], v["fc3.bias"])
    losses = F.cross_entropy(z, ref["y"], reduction="none")
    (losses.sum() * case.grad_scale).backward()
    assert torch.equal(z.detach(), ref["z"])
    assert float((losses.detach() - ref["loss"]).abs().max()) <= 1e-12 * float(ref["loss"].abs().max())
    # m = 8: torch's probabilities are exp(-fl(ln 8)), an ulp of float64 off 1/8 (ln 2 and ln 4 happen to
    # round-trip), which the backward sums carry: a few 2^-53 of each GEMM's sum of absolute terms
    tol = 1e-13 if case.name == "T128" else 1e-30
    for name, shape, off, n in M.param_layout():
        a, b = flat.grad[off:off + n], ref["grad"][off:off + n]
        assert float((a - b).abs().max()) <= tol * float(b.abs().max()), name
    assert torch.equal(ref["correct"], (ref["z"].argmax(1) == ref["y"]).double())  # (argmax: the first maximum)
    p = torch.nn.Parameter(o["flat"].double().clone())
    opt = torch.optim.SGD([p], lr=X.LR, momentum=X.MU, weight_decay=X.WD)
    opt.state[p]["momentum_buffer"] = o["mom0"].double().clone()
    p.grad = ref["grad"].clone()
    opt.step()
    assert torch.equal(p.detach(), ref["params"]) and torch.equal(opt.state[p]["momentum_buffer"], ref["mom"])


def test_loss_bound_is_the_derived_one():
    ref = X.reference(X.CASES_BY_NAME["S128"])
    assert float(X.ulp32(torch.tensor([1.0, 3.0, 65536.0 + 5], dtype=torch.float64))[2]) == 2.0 ** -7
    zl = ref["z"].gather(1, ref["y"][:, None])[:, 0]
    mx = ref["z"].max(1).values
    want = X.ulp32(torch.maximum(mx.abs(), zl.abs()) + 3.0) + 4 * 2.0 ** -22
    assert torch.equal(ref["loss_bound"], want)
    # the rows whose label is among the maxima have loss ln m, the others at least 128 more
    among = (ref["ismax"] & F.one_hot(ref["y"], 10).bool()).any(1)
    assert torch.allclose(ref["loss"][among], torch.log(ref["m"][among].double()), rtol=0, atol=1e-9)
    assert float(ref["loss"][~among].min()) >= 128.0


def test_frag_index_is_the_inverse_of_the_shadow_layout():
    """frag_off of mlp_fused.hip: block (n / 16, k / 32) of 512 elements, lane 16 (k % 32 / 8) + n % 16,
    element k % 8; decode_frag reads a matrix back and counts what lies outside it."""
    idx = X.frag_index(256, 784, X.KS1)
    assert idx.unique().numel() == 256 * 784 and int(idx.max()) < 256 * M.D_IN_PAD
    assert int(idx[0, 0]) == 0 and int(idx[1, 0]) == 8 and int(idx[0, 8]) == 128 and int(idx[0, 32]) == 512
    assert int(idx[16, 0]) == X.KS1 * 512 and int(idx[17, 41]) == (X.KS1 + 1) * 512 + (16 + 1) * 8 + 1
    mat = torch.arange(10 * 256, dtype=torch.float32).view(10, 256) + 1
    buf = torch.zeros(16 * 256)
    buf[X.frag_index(10, 256, X.KS2).reshape(-1)] = mat.reshape(-1)
    got, rest = X.decode_frag(buf, 10, 256, X.KS2)
    assert torch.equal(got, mat) and rest == 0
    buf[X.frag_index(16, 256, X.KS2)[12, 3]] = 5.0  # a padding row of w3h
    assert X.decode_frag(buf, 10, 256, X.KS2)[1] == 1
    assert int(X.frag_index(256, 10, 1).max()) < 256 * 32


def test_comparator_messages():
    ref = X.reference(X.CASES_BY_NAME["S128"])
    good = ref["dh2"].to(torch.bfloat16)  # what a correct kernel stores
    assert X.compare(good, ref["dh2"], "dh2t", bm=128) is None
    bad = good.clone()
    r, c = [int(v) for v in (ref["dh2"] != 0).nonzero()[40]]
    bad[r, c] = 0
    bad[127, 255] = float("nan")
    m = X.compare(bad, ref["dh2"], "dh2t", bm=128)
    assert (m.what, m.count, m.total, m.index, m.got, m.want) == ("dh2t", 2, 128 * 256, (r, c), 0.0, float(ref["dh2"][r, c]))
    text = str(m)
    assert text.startswith("dh2t: 2 of 32768 elements differ; first at (%d, %d): got 0.0, want " % (r, c))
    assert "rows workgroup 0 row %d (fragment row %d), wave %d column %d" % (r, r % 16, c // 64, c % 64) in text
    late = good.clone()
    late[70, 200] += 1  # the same buffer from 64-row workgroups
    assert "rows workgroup 1 row 6 (fragment row 6), wave 3 column 8" in str(X.compare(late, ref["dh2"], "dh2t", bm=64))
    # a bound instead of equality (the loss): inside passes, outside names the bound
    lb = ref["loss_bound"]
    assert X.compare(ref["loss"] + 0.999 * lb, ref["loss"], "loss", bound=lb) is None
    off = ref["loss"].clone()
    off[77] += 1.5 * lb[77]
    m = X.compare(off, ref["loss"], "loss", bound=lb)
    assert m.count == 1 and m.index == (77,) and "bound %r" % float(lb[77]) in str(m)
    # a flat vector: tensor by tensor, index within the tensor
    g = ref["grad"].clone()
    off2 = [o for n, s, o, _ in M.param_layout() if n == "fc2.weight"][0]
    g[off2 + 3 * 256 + 9] += 1
    (m,) = X.compare_flat(g, ref["grad"], "grad")
    assert m.what == "grad fc2.weight" and m.index == (3, 9) and m.count == 1 and m.got == m.want + 1


# ---------------------------------------------------------------------------------------------
# five localized faults: what the norm-wise bounds say, and what the exact comparison says
# ---------------------------------------------------------------------------------------------
OFF = {n: (o, s) for n, s, o, _ in M.param_layout()}


def _t(flat, name):
    o, s = OFF[name]
    return flat[o:o + torch.Size(s).numel()]


def _t2(flat, name):
    return _t(flat, name).view(OFF[name][1])


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _fp32_bounds(g, gref):
    """test_gradients_match_reference against the fp32 autograd gradient: cosine and 5e-2."""
    return all(float(F.cosine_similarity(_t(g, n), _t(gref, n), dim=0)) > 0.995
               and float((_t(g, n) - _t(gref, n)).norm() / _t(gref, n).norm()) < 5e-2 for n in OFF)


def _emu_bounds(g, gemu):
    """... against the emulation that rounds where the kernels round: 5e-3 in norm, 2e-2 of the maximum."""
    return all(float((_t(g, n) - _t(gemu, n)).norm() / _t(gemu, n).norm()) < 5e-3 and _rel(_t(g, n), _t(gemu, n)) < 2e-2
               for n in OFF)


def _sgd_step_bound(flat, g, gref, wd=1e-4, wd_ref=1e-4):
    """test_sgd_step_matches_reference: cosine of the weight deltas above 0.995."""
    got, ref = flat.clone(), flat.clone()
    M.sgd_update(got, torch.zeros_like(got), g, 0.1, 0.9, wd)
    M.sgd_update(ref, torch.zeros_like(ref), gref, 0.1, 0.9, wd_ref)
    return float(F.cosine_similarity(got - flat, ref - flat, dim=0)) > 0.995


def _column_shift(g):  # dW1 column 300 holds column 301
    _t2(g, "fc1.weight")[:, 300] = _t2(g, "fc1.weight")[:, 301].clone()


def _db2_rotate(g):  # every lane of db2 holds its neighbour's value
    _t(g, "fc2.bias").copy_(torch.roll(_t(g, "fc2.bias").clone(), 1))


@functools.lru_cache(maxsize=None)
def _mnist_like():
    """The inputs of the norm-wise tests (batch 512): the fp32 gradient they compare with, the
    emulated one a correct kernel delivers, and the emulated gradient of rows 64..127 alone (one
    64-row split-K slice)."""
    b = 512
    x, y = make_mnist_like(b, seed=5)
    x, y = torch.from_numpy(x), torch.from_numpy(y)
    flat = M.init_params(4)
    gref = M.reference_grads(flat, x, y, 1.0 / b)[2]
    gemu = M.reference_grads_bf16(flat, x, y, 1.0 / b)[2]
    part = M.reference_grads_bf16(flat, x[64:128], y[64:128], 1.0 / b)[2]
    return flat, gref, gemu, part


def test_record_what_the_norm_bounds_say_to_five_faults():
    """On the norm-wise tests' own inputs.  Every one of the five passes the only independent check
    of the default update (test_sgd_step_matches_reference, cosine > 0.995 of the weight delta).
    test_gradients_match_reference's bounds against the rounding emulation (5e-3 in norm, 2e-2 of
    the largest element) do reject the three gradient faults at this batch -- one of 784 columns is
    already 3 % of dW1's norm -- and never see the other two, which are not in the gradient."""
    flat, gref, gemu, part = _mnist_like()
    assert _fp32_bounds(gemu, gref) and _emu_bounds(gemu, gemu) and _sgd_step_bound(flat, gemu, gref)
    faults = {}
    g = gemu.clone()
    _column_shift(g)
    faults["one dW1 column shifted by one"] = g
    g = gemu.clone()
    _t2(g, "fc2.weight")[5] -= _t2(part, "fc2.weight")[5]  # row 5 of dW2 lost the rows of one slice
    faults["one slice's rows dropped"] = g
    g = gemu.clone()
    _db2_rotate(g)
    faults["db2 rotated by one lane"] = g
    for name, g in faults.items():
        assert not torch.equal(g, gemu), name
        assert _sgd_step_bound(flat, g, gref), name
        print(name, "-- against the fp32 gradient (cosine, 5e-2):", "accepted" if _fp32_bounds(g, gref) else "rejected")
        assert not _emu_bounds(g, gemu), name
    # weight decay ignored: the update's fault, invisible to every gradient check
    assert _sgd_step_bound(flat, gemu, gref, wd=0.0)
    got = flat.clone()
    M.sgd_update(got, torch.zeros_like(got), gemu, 0.1, 0.9, 0.0)
    ref = flat.clone()
    M.sgd_update(ref, torch.zeros_like(ref), gemu, 0.1, 0.9, 1e-4)
    assert not torch.equal(got, ref)
    # one W2 shadow entry stale: the parameters of a one-step test do not depend on the shadows at all


def test_record_the_exact_comparison_rejects_and_locates_them():
    """The same five, injected into what a correct kernel delivers for a case: each is a mismatch,
    and the message names the tensor and the place."""
    case = X.CASES_BY_NAME["S384"]
    ref = X.reference(case)
    good = ref["grad"].float()
    assert X.compare_flat(good, ref["grad"], "grad") == []

    g = good.clone()
    _column_shift(g)
    (m,) = X.compare_flat(g, ref["grad"], "grad")
    w1 = _t2(ref["grad"], "fc1.weight")
    assert m.what == "grad fc1.weight" and m.index[1] == 300 and m.count == int((w1[:, 300] != w1[:, 301]).sum()) > 128

    # slice 1 of the three (rows 128..255) dropped from row 5 of dW2
    sl = slice(128, 256)
    g = good.clone()
    _t2(g, "fc2.weight")[5] -= (ref["dh2"][sl, 5] @ ref["h1"][sl]).float()
    (m,) = X.compare_flat(g, ref["grad"], "grad")
    assert m.what == "grad fc2.weight" and m.index[0] == 5 and m.count > 128

    g = good.clone()
    _db2_rotate(g)
    (m,) = X.compare_flat(g, ref["grad"], "grad")
    assert m.what == "grad fc2.bias" and m.count > 192
    part = ref["w3p"].float()
    part[1, X.W3P_DB2:] = torch.roll(part[1, X.W3P_DB2:].clone(), 1)  # ... or in one workgroup's partial row only
    m = X.compare(part[:, X.W3P_DB2:], ref["w3p"][:, X.W3P_DB2:], "w3p partial rows, db2")
    assert m is not None and m.index[0] == 1

    o = X.operands(case)
    w0, m0 = o["flat"].double(), o["mom0"].double()
    no_wd = w0 - X.LR * (X.MU * m0 + ref["grad"])
    bad = X.compare_flat(no_wd.float(), ref["params"], "params")
    assert [m.what for m in bad] == ["params " + n for n in OFF]  # every tensor has non-zero weights
    assert bad[0].count == int((_t(w0, "fc1.weight") != 0).sum())

    stale = ref["w2h"].clone()
    stale[17, 33] = float(_t2(w0, "fc2.weight")[17, 33])
    m = X.compare(stale, ref["w2h"], "w2h (decoded)")
    assert m is not None and m.count == 1 and m.index == (17, 33)
    assert X.compare(ref["w2h"].to(torch.bfloat16), ref["w2h"], "w2h (decoded)") is None
