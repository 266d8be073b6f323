"""The rows kernel's epilogues, position by position: the softmax cross-entropy (one batch row
per lane quarter: per-sample loss, correctness, logits, ties) and the 128-row tile's dH1
(16-byte stores of fragment pairs loaded through a permuted lane map) with its db1 partial.

The whole-gradient tests would pass a wrong row or column assignment that happens to cancel in
a sum over the batch; here every sample and every (row, feature) is compared on its own."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from serverless_learn_amd.data.synthetic import make_mnist_like
from serverless_learn_amd.models import mlp as M

pytestmark = pytest.mark.gpu

W3P_DB1 = 2576  # column of the db1 partial in a rows-kernel partial row (mlp_fused.hip)


@pytest.fixture
def rows_bm():
    from serverless_learn_amd.ops import _native

    yield lambda bm: _native.call("sl_mlp_set_rows_bm", bm)
    _native.call("sl_mlp_set_rows_bm", 0)


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@functools.lru_cache(maxsize=None)
def _case(n):
    """(x, y, flat, reference) for a batch of n; computed once, never modified."""
    x, y = make_mnist_like(n, seed=5 if n == 384 else 3)
    x, y = torch.from_numpy(x), torch.from_numpy(y)
    assert set(y.tolist()) == set(range(M.CLASSES)), "every label occurs"
    flat = M.init_params(2)
    return x, y, flat, _reference_bf16(flat, x, y, 1.0 / n)


def _reference_bf16(flat, x_u8, y, grad_scale):
    """M.reference_grads_bf16's forward and backward down to dH1, in float64 between the bf16
    rounding points (so the reference does not depend on the host's summation order).
    Returns per-sample / per-element values: z, losses, dh1, and dh1_slack: how far dH1 may
    legitimately move where a ReLU decision of the reference is within rounding of zero."""
    r = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    v = {k: t.detach().double() for k, t in M.views(flat).items()}
    a, b = M.norm_coeffs()
    xu = x_u8.reshape(-1, M.D_IN).double()
    xe = xu * a + b
    w1 = v["fc1.weight"].to(torch.float16).double()
    w2, w3 = r(v["fc2.weight"]), r(v["fc3.weight"])
    p1 = xe @ w1.t() + v["fc1.bias"]
    h1 = r(torch.relu(p1))
    p2 = h1 @ w2.t() + v["fc2.bias"]
    h2 = r(torch.relu(p2))
    z = h2 @ w3.t() + v["fc3.bias"]
    yl = y.reshape(-1).long()
    losses = torch.logsumexp(z, 1) - z.gather(1, yl[:, None])[:, 0]
    dz = r((torch.softmax(z, 1) - F.one_hot(yl, M.CLASSES).double()) * grad_scale)
    pre2 = dz @ w3
    dh2 = r(pre2 * (p2 > 0).double())
    pre1 = dh2 @ w2
    dh1 = pre1 * (p1 > 0).double()  # the 128-row tile stores fp16 of the fp32 product
    # ReLU decisions the kernel may take the other way, from the number formats alone:
    # layer 1 sums 784 exact products (1024 + u) * w1 in fp32 and scales by a: 2^-24 relative
    # per addition, the 784 roundings adding like a random walk (sqrt(784); the worst case,
    # 784, would put half of all elements in doubt); layer 2 sees H1 rounded to bf16 (2^-9
    # relative), one element of which on the other side of a rounding boundary moves p2 by up
    # to 2^-9 max|h1| max|w2|, plus layer 1's own doubt through w2.  A flipped layer-2 decision
    # (row, k) moves dH1[row, :] by pre2[row, k] * w2[k, :]; a flipped layer-1 decision sets
    # or clears the element itself.
    d1 = math.sqrt(M.D_IN) * 2.0 ** -24 * float(((1024.0 + xu) @ w1.abs().t()).max()) * a
    d2 = 2.0 ** -9 * float(h1.max()) * float(w2.abs().max()) + d1 * float(w2.abs().max())
    slack = ((p2.abs() < d2).double() * pre2.abs()) @ w2.abs() + (p1.abs() < d1).double() * pre1.abs()
    return {"z": z.float(), "losses": losses.float(), "dh1": dh1.float(), "dh1_slack": slack.float()}


# Worst per-sample |loss - reference| of the commit before the lane-per-row softmax, measured
# on these inputs on an MI355X (the new form is bit-identical to it); the bound is twice that.
PARENT_LOSS_DEV = {128: 4.909e-04, 384: 3.567e-04, 64: 2.313e-04, 192: 2.165e-04}


@pytest.mark.parametrize("batch,bm", [(128, 128), (384, 128), (64, 64), (192, 64)])
def test_per_sample_loss_correct_logits(batch, bm, rows_bm):
    from serverless_learn_amd.ops import _native

    rows_bm(bm)
    assert _native.lib().sl_mlp_rows_bm(batch) == bm
    x, y, flat, ref = _case(batch)
    tr = M.FusedMLPTrainer(batch=batch, flat=flat, momentum=0.0)
    tr.load_shard(x, y)
    tr.compute_grads()
    torch.cuda.synchronize()
    loss, correct = tr.loss.cpu(), tr.correct.cpu()
    logits = tr.logits(x).cpu()

    z = ref["z"]
    rz, rf = _rel(logits, z), _rel(logits, M.MLP(flat)(x).detach())
    dev = float((loss - ref["losses"]).abs().max())
    print(f"batch {batch} bm {bm}: logits rel vs bf16 reference {rz:.3e}, vs fp32 {rf:.3e}; "
          f"worst per-sample loss deviation {dev:.3e}")
    assert rz < 3e-2 and rf < 3e-2, (rz, rf)
    assert dev <= 2 * PARENT_LOSS_DEV[batch], (dev, int((loss - ref["losses"]).abs().argmax()))

    top2 = z.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) >= 1e-3
    assert int((~clear).sum()) <= 0.05 * batch
    want = (z.argmax(1) == y.long()).float()
    bad = ((correct != want) & clear).nonzero()
    assert bad.numel() == 0, f"correct differs first at row {int(bad[0])}"


@pytest.mark.parametrize("batch,bm", [(128, 128), (64, 64)])
def test_ties_take_the_first_class(batch, bm, rows_bm):
    """All ten logits equal (W3 = 0, b3 = 0): the prediction is class 0, the first of the
    maxima, and the loss is log(10)."""
    rows_bm(bm)
    x, y, flat, _ = _case(batch)
    flat = flat.clone()
    v = M.views(flat)
    v["fc3.weight"].zero_()
    v["fc3.bias"].zero_()
    tr = M.FusedMLPTrainer(batch=batch, flat=flat, momentum=0.0)
    tr.load_shard(x, y)
    tr.compute_grads()
    torch.cuda.synchronize()
    assert torch.equal(tr.correct.cpu(), (y == 0).float())
    # the kernel's log is v_log_f32 (1 ulp at log2(10) = 3.32, i.e. 2.4e-7) times ln 2, rounded,
    # on an exact sum of ten ones: within 4 fp32 ulps of 2.3026 (ulp 2.4e-7)
    dev = float((tr.loss.cpu().double() - math.log(10.0)).abs().max())
    print(f"batch {batch}: worst |loss - log 10| {dev:.3e}")
    assert dev <= 4 * 2.0 ** -22, dev


@pytest.mark.parametrize("batch", [128, 256])
def test_dh1_position_and_db1_partial(batch, rows_bm):
    from serverless_learn_amd.ops import _native

    rows_bm(128)
    assert _native.lib().sl_mlp_rows_bm(batch) == 128
    x, y, flat, ref = _case(batch)
    tr = M.FusedMLPTrainer(batch=batch, flat=flat, momentum=0.0)
    tr.load_shard(x, y)
    tr.w3p.zero_()  # one partial row per workgroup is written; the buffer has one per 64 rows
    tr._rows(True)
    torch.cuda.synchronize()
    got = (tr.dh1t.view(torch.float16).float() / tr.dh1_scale).cpu()
    dh1, slack = ref["dh1"], ref["dh1_slack"]
    # the gradient test's bound, relative to the largest element; where a ReLU decision of the
    # reference is within rounding of zero (_reference_bf16), plus what that decision moves
    scale = float(dh1.abs().max()) + 1e-12
    err = (got - dh1).abs()
    bad = (err >= 2e-2 * scale + slack).nonzero()
    clean = slack == 0
    print(f"batch {batch}: dH1 rel {float(err[clean].max()) / scale:.3e} over the {float(clean.float().mean()):.1%} "
          f"of elements without slack; worst (err - slack) / max {float((err - slack).max()) / scale:.3e}")
    assert float(clean.float().mean()) > 0.5  # the reference alone: 70.3 % / 76.9 % here
    assert bad.numel() == 0, f"dH1 differs first at (row, column) {tuple(bad[0].tolist())}: " \
                             f"{float(got[tuple(bad[0])])} vs {float(dh1[tuple(bad[0])])}"
    db1 = tr.w3p[:, W3P_DB1:W3P_DB1 + M.HIDDEN].sum(0).cpu()
    want = dh1.sum(0)
    rn = float((db1 - want).norm() / want.norm())
    print(f"batch {batch}: db1 partial relative norm error {rn:.3e}")
    assert rn < 5e-3, rn
