"""The exact-convolution checker checked on the CPU (serverless_learn_amd/utils/conv_exact.py): its
float64 reference against torch's own convolution and autograd, its operand bounds, and that its
comparator sees -- and locates -- the localized faults the norm-wise ``rel`` of
tests/test_cnn_gpu.py lets through.  That last test is why tests/test_conv_exact_gpu.py exists."""
import functools

import pytest
import torch
import torch.nn.functional as F

from serverless_learn_amd.ops.cnn import KERNEL_FAMILIES
from serverless_learn_amd.utils import conv_exact as X

SMALL = [c for c in X.CASES if c.cpu_sized()]


def rel(a, b):
    """The norm-wise measure of tests/test_cnn_gpu.py."""
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / (b.norm() + 1e-12))


@functools.lru_cache(maxsize=None)
def _ref(name):
    case = X.CASES_BY_NAME[name]
    o = X.operands(case, "cpu")
    return o, X.case_reference(case, o)


def test_case_table_is_consistent():
    assert {c.group for c in X.CASES} == set("ABCDEFG")
    for c in X.CASES:
        fams = set(c.fwd) | set(c.dgrad) | set(c.wgrad) | {f for part in c.smallm for f in part}
        assert fams <= set(KERNEL_FAMILIES), (c.name, fams - set(KERNEL_FAMILIES))
        assert c.fwd and c.wgrad and (c.dgrad or not c.do_dgrad), c.name
        assert not c.even or (c.shape[6] == 2 and c.shape[5] in (1, 3)), c.name
    # every family the table can reach by shape alone is the named target of at least one case
    named = {f for c in X.CASES for part in (c.fwd, c.dgrad, c.wgrad, *c.smallm) for f in part}
    assert named == set(KERNEL_FAMILIES) - {"wide128", "wide128_t", "dgrad_s2_alt"}, named  # A/B-knob tile shapes
    for sub in X.SUBSETS.values():
        assert sub and all(n in X.CASES_BY_NAME for n in sub)
    assert {X.CASES_BY_NAME[n].group for n in X.SUBSETS["det"]} == set("BCDFG")
    # the cases too large for the CPU are the ones the GPU test bounds on the device
    assert len(SMALL) >= 20 and any(not c.cpu_sized() for c in X.CASES)


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_reference_matches_torch_float64(case):
    """Forward, dX and dW of the tap-by-tap reference equal torch's conv2d and its autograd in
    float64 -- exactly, the operands being integers."""
    n, h, w, c, cout, k, s, p = case.shape
    o, ref = _ref(case.name)
    xr = o["x"].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr = o["w"].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=s, padding=p)
    y.backward(o["dy"].double().permute(0, 3, 1, 2))
    assert torch.equal(ref["y"], y.detach().permute(0, 2, 3, 1))
    assert torch.equal(ref["dx"], xr.grad.permute(0, 2, 3, 1))
    assert torch.equal(ref["dw"] - o["dw0"].double(), wr.grad.permute(0, 2, 3, 1))
    if case.even and k == 3:  # the 1x1 / stride-2 shortcut's gradient sits at the even positions
        xs = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
        ys = F.conv2d(xs, o["wsc"].double().view(cout, c, 1, 1), stride=2)
        ys.backward(o["dys"].double().permute(0, 3, 1, 2))
        assert torch.equal(ref["dx_even"], (xr.grad + xs.grad).permute(0, 2, 3, 1))
        assert torch.equal(ref["even"], xs.grad.permute(0, 2, 3, 1)[:, ::2, ::2])


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_bounds_hold(case):
    """|bf16 outputs| <= 256 and |fp32 outputs| < 2^24 on the reference, with margin."""
    _, ref = _ref(case.name)
    m = X.check_bounds(case, ref)
    assert max(m[k] for k in m if k not in ("stats", "dw")) <= 128, m
    assert max(m["stats"], m["dw"]) < 2 ** 22, m


def test_operands_are_small_integers_at_the_case_density():
    case = X.CASES_BY_NAME["A1-3x7x7-128-256"]
    o = X.operands(case, "cpu")
    for key, lim in (("x", 2), ("dy", 2), ("add", 2), ("w", 1)):
        v = o[key].double()
        assert torch.equal(v, v.round()) and float(v.abs().max()) == lim, key
    assert abs(float((o["w"] != 0).double().mean()) - case.density() * 2 / 3) < 0.02
    assert abs(float((o["x"] != 0).double().mean()) - case.density() * 4 / 5) < 0.02
    big = X.CASES_BY_NAME["D4-1024x16x16-128-256-s2"]
    assert case.density() == 0.25 and big.density() == 0.125 and not big.cpu_sized()


def test_comparator_sees_what_the_norm_misses():
    """One element off by 1, one zeroed border pixel, two rows swapped inside one 16-row MFMA
    fragment, in a 65,536-row output: each passes rel(...) < 1e-2, the measure of every existing
    convolution test, and each fails the comparator, which names the place."""
    case = X.Case("sens", (64, 32, 32, 8, 64, 3, 1, 1))
    o = X.operands(case, "cpu")
    ref, _, _ = X.reference(o["x"], o["w"], o["dy"], 1, 1)
    n, hh, ww, ch = ref.shape
    assert n * hh * ww == 65536
    good = ref.to(torch.bfloat16)  # what a correct kernel stores
    assert X.compare(good, ref) is None

    one = good.clone()
    one[17, 5, 9, 33] += 1
    m = X.compare(one, ref, "y")
    assert rel(one, ref) < 1e-2
    assert m is not None and m.count == 1 and m.index == (17, 5, 9, 33) and m.got == m.want + 1
    row = (17 * 32 + 5) * 32 + 9
    assert m.row == row and m.tiles == {256: (row // 256, row % 256), 128: (row // 128, row % 128),
                                        64: (row // 64, row % 64)}
    assert "GEMM row %d" % row in str(m) and "(17, 5, 9, 33)" in str(m)

    border = good.clone()
    assert int((ref[40, 0, 31] != 0).sum()) > 8
    border[40, 0, 31] = 0
    m = X.compare(border, ref, "y")
    assert rel(border, ref) < 1e-2
    assert m is not None and m.index[:3] == (40, 0, 31) and m.count == int((ref[40, 0, 31] != 0).sum())
    assert m.row == 40 * 1024 + 31 and m.got == 0.0 and m.want != 0.0

    swap = good.clone().view(-1, ch)
    frag = 1234
    r0, r1 = frag * 16 + 3, frag * 16 + 9
    assert not torch.equal(swap[r0], swap[r1])
    swap[[r0, r1]] = swap[[r1, r0]]
    swap = swap.view(ref.shape)
    m = X.compare(swap, ref, "y")
    assert rel(swap, ref) < 1e-2
    assert m is not None and m.row == r0 and m.row % 16 == 3 and m.tiles[256] == (r0 // 256, r0 % 256)
    assert m.count == 2 * int((good.view(-1, ch)[r0] != good.view(-1, ch)[r1]).sum())
    assert "fragment row 3" in str(m)

    unwritten = good.clone()
    unwritten[63, 31, 31, 63] = float("nan")
    m = X.compare(unwritten, ref, "y")
    assert m is not None and m.count == 1 and m.index == (63, 31, 31, 63)


def test_comparator_decodes_parity_classes():
    """A stride-2 data gradient's pixel (oh, ow) belongs to class (oh & 1, ow & 1), which has its
    own row numbering (odd extents: unequal classes)."""
    ref = torch.zeros(3, 7, 7, 8, dtype=torch.float64)
    got = ref.clone()
    got[2, 5, 4, 1] = 1
    m = X.compare(got, ref, "dx", parity=True)
    assert m.index == (2, 5, 4, 1) and m.cls == (1, 0)
    assert m.cls_row == (2 * 3 + 2) * 4 + 2 and m.cls_tiles[64] == (0, m.cls_row)  # class (1, 0): 3 x 4 pixels
    assert m.row == (2 * 7 + 5) * 7 + 4 and "parity class (1, 0)" in str(m)
    stats = X.compare(torch.tensor([1.0, 2.0, 4.0]), torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64), "s", pixels=False)
    assert stats.index == (2,) and stats.row == -1 and stats.cls == ()
