"""Held-out evaluation on the GPU: ``eval_accum_kernel`` (csrc/kernels/eval_metrics.hip, ops/evalmetrics.py
eval_accum) against its definition ``eval_reference``, and ``evaluate_full`` in both training engines.

Everything the kernel accumulates is an integer -- counts, the confusion matrix, the loss as
``rint(loss * 2^24)`` -- so every comparison here is an equality of all 264 words of the device block, and
the result does not depend on the order in which workgroups add.  For the same reason the kernel has no
``SL_DETERMINISTIC`` branch (checked by reading eval_metrics.hip: no float atomic, no ticket, no ``#if``), so
its cases run through the library this process loaded; the default and the deterministic build compile the
same code.  The ResNet engine's cases run in one ``SL_DETERMINISTIC=1`` child (scripts/eval_resnet_det.py):
the comparison with a twin trainer that never evaluated needs bit-reproducible training steps, as in
tests/test_ema_gpu.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from serverless_learn_amd.ops import evalmetrics as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ROWS = 53  # 3 full workgroups of 16 rows plus 5
NAN, INF = float("nan"), float("inf")


def _block(rep: E.EvalReport) -> np.ndarray:
    """The device block a report corresponds to: counters, three zero words, the 16 x 16 confusion matrix."""
    a = np.zeros(E.ACC_LEN, np.int64)
    a[:5] = (rep.n, rep.bad, rep.top1, rep.topk, rep.loss_fix)
    ncls = rep.confusion.shape[0]
    conf = np.zeros((16, 16), np.int64)
    conf[:ncls, :ncls] = rep.confusion
    a[E.ACC_HEAD:] = conf.reshape(-1)
    return a


def _case(rows: int, ncls: int, seed: int = 0):
    """(logits [rows, ncls], labels, loss rows) on the host: logits from the integer grid -2..2 (ties are
    frequent), arbitrary positive losses, and the planted rows of the module's cases."""
    g = torch.Generator().manual_seed(seed + 131 * ncls + rows)
    z = torch.randint(-2, 3, (rows, ncls), generator=g).float()
    lab = torch.randint(0, ncls, (rows,), generator=g).to(torch.uint8)
    loss = (torch.rand(rows, generator=g) * 5).float()
    if rows >= ROWS:
        z[0] = 0.0
        z[0, 0] = z[0, 2] = 3.0
        lab[0] = 2                   # the maximum ties include the label, at a higher index: pred 0, rank 1
        z[1] = 0.0
        z[1, 1] = z[1, 4] = 3.0
        lab[1] = 1                   # ... at the lowest index: pred 1, rank 0
        z[2, 3] = NAN                # bad rows: a NaN logit,
        z[3, ncls - 1] = INF         # a +inf logit,
        loss[4] = NAN                # a NaN loss,
        loss[5] = 65536.0            # a loss of exactly 2^16
        loss[6] = -1e-7              # a tiny negative loss: good, rounds to -2 units
        lab[7] = 200 if ncls == 16 else ncls  # a label >= ncls counts as 0
        loss[17] = 65535.996         # the largest fp32 below 2^16: good
        z[20, 0] = NAN               # bad rows in the later workgroups too
        z[40, 1] = -INF
        loss[50] = -INF
        loss[51] = -65536.0
    return z, lab, loss


def _launch(z, lab, loss, n_valid, ncls, topk, acc=None, ld=None):
    """The rows on the device with everything from row n_valid on made unreadable (NaN logits and loss,
    label 255); the logits as a view of a [rows, ld] buffer when ``ld`` is given."""
    zd, ld_, lo = z.clone(), lab.clone(), loss.clone()
    zd[n_valid:] = NAN
    lo[n_valid:] = NAN
    ld_[n_valid:] = 255
    if ld is not None:
        buf = torch.full((z.shape[0], ld), NAN)
        buf[:, :ncls] = zd
        zd = buf.to(DEV)[:, :ncls]
    else:
        zd = zd.to(DEV)
    acc = E.new_acc(DEV) if acc is None else acc
    E.eval_accum(zd, ld_.to(DEV), lo.to(DEV), n_valid, ncls, topk, acc)
    return acc


# ---- 1. the kernel ----
@pytest.fixture(scope="module")
def cases():
    return {ncls: _case(ROWS, ncls) for ncls in (10, 16)}


@pytest.mark.parametrize("n_valid", [53, 37, 16, 1, 0])
@pytest.mark.parametrize("topk", [1, 5, "ncls"])
@pytest.mark.parametrize("ncls", [10, 16])
def test_kernel_equals_the_definition(cases, ncls, topk, n_valid):
    topk = ncls if topk == "ncls" else topk
    z, lab, loss = cases[ncls]
    want = E.eval_reference(z[:n_valid], lab[:n_valid], loss[:n_valid], ncls, topk)
    acc = _launch(z, lab, loss, n_valid, ncls, topk)
    got = acc.cpu().numpy()
    print(ncls, topk, n_valid, got[:8], want.as_dict()["loss"])
    assert np.array_equal(got, _block(want)), (got[:8], _block(want)[:8])
    assert E.report_from_acc(acc, ncls, topk) == want
    if n_valid == ROWS:  # every planted row took part
        assert want.bad == 8 and want.n == ROWS and int(want.confusion.sum()) == ROWS - 8
        assert want.confusion[2, 0] >= 1 and want.confusion[1, 1] >= 1 and want.confusion[0].sum() >= 1
        assert (want.topk == want.top1) if topk == 1 else (want.topk > want.top1)
        assert (want.topk == want.n - want.bad) if topk == ncls else True
    # adds, never overwrites: a second launch without zeroing doubles every field
    _launch(z, lab, loss, n_valid, ncls, topk, acc=acc)
    assert np.array_equal(acc.cpu().numpy(), 2 * _block(want))
    # the logits' row stride is an argument: the same rows inside a [rows, 16] buffer whose other columns are NaN
    if ncls == 10:
        assert np.array_equal(_launch(z, lab, loss, n_valid, ncls, topk, ld=16).cpu().numpy(), _block(want))


def test_many_workgroups_add_onto_the_same_bins():
    rows, ncls, topk = 4099, 10, 5
    z, lab, loss = _case(rows, ncls, seed=1)
    z[::97, 3] = NAN
    loss[5::211] = INF
    loss[7::13] *= -1.0
    want = E.eval_reference(z, lab, loss, ncls, topk)
    a, b = _launch(z, lab, loss, rows, ncls, topk), _launch(z, lab, loss, rows, ncls, topk)
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), _block(want)), (a[:8].tolist(), _block(want)[:8])
    assert want.bad > 40 and want.loss_fix != 0 and int(want.confusion.sum()) == rows - want.bad


def test_entry_point_refuses_bad_arguments():
    z, lab, loss = (t.to(DEV) for t in _case(32, 10))
    acc = E.new_acc(DEV)
    for kw in (dict(ncls=17), dict(ncls=0), dict(topk=0), dict(topk=11), dict(n_valid=33), dict(n_valid=-1)):
        a = dict(n_valid=32, ncls=10, topk=5)
        a.update(kw)
        with pytest.raises(RuntimeError, match="sl_eval_accum"):
            E.eval_accum(z, lab, loss, a["n_valid"], a["ncls"], a["topk"], acc)
    with pytest.raises(RuntimeError, match="sl_eval_accum"):  # a row stride shorter than the classes
        E.eval_accum(z[:, :8].contiguous(), lab, loss, 32, 10, 5, acc)
    with pytest.raises(TypeError):
        E.eval_accum(z.double(), lab, loss, 32, 10, 5, acc)
    assert int(acc.abs().sum()) == 0  # nothing was launched


# ---- 2. the MLP engine ----
B = 256
N_MLP = 64 * 3 + 9
TRAINING = ("params", "mom", "v", "w1h", "w2h", "w2th", "w3h", "w3th", "r1p", "opt_step", "opt_ticket", "cursor",
            "grad", "loss", "correct", "clip_norm", "ema", "ema_step", "ema_ticket")


def _mnist(n: int, seed: int):
    from serverless_learn_amd.data.synthetic import make_mnist_like

    x, y = make_mnist_like(n, seed=seed)
    return torch.from_numpy(x), torch.from_numpy(y)


def _rows_launch(tr, xp, yp, ema=False):
    """(logits, per-row loss) of padded rows: ``logits()`` and the launch ``evaluate()`` makes for its loss."""
    n, s = tr._n, tr._eval_set(ema)
    xd, yd = xp.to(DEV).contiguous(), yp.to(DEV).contiguous()
    rows = xd.shape[0]
    loss, corr = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
    n.call("sl_mlp_rows", n.ptr(xd), n.ptr(yd), None, 1, rows,
           n.ptr(s["w1h"]), n.ptr(s["w2h"]), n.ptr(s["w3h"]), n.ptr(s["w2th"]), n.ptr(s["w3th"]),
           n.ptr(s["params"]), tr.xa, tr.xb, 1.0, 1.0, None, None, None, None,
           n.ptr(loss), n.ptr(corr), None, 0, n.ptr(s["r1p"]), None, n.stream_ptr())
    return tr.logits(xp, ema=ema).cpu(), loss.cpu()


def test_mlp_evaluate_full_covers_every_record_and_leaves_training_alone():
    from serverless_learn_amd.models.mlp import D_IN, FusedMLPTrainer

    tr = FusedMLPTrainer(batch=B, device=DEV, seed=1, ema_decay=0.5, lr=0.05, momentum=0.9)
    tr.load_shard(*_mnist(4 * B, 3))
    tr.capture(warmup=0, unroll=4)
    tr.steps(6)
    torch.cuda.synchronize()
    x, y = _mnist(N_MLP, 4)
    y[5] = 10  # a label >= ncls: counted as class 0, as the rows kernel's loss does
    names = [n for n in TRAINING if getattr(tr, n) is not None]
    before = {n: getattr(tr, n).clone() for n in names}
    ptrs = {n: getattr(tr, n).data_ptr() for n in names}
    rep, avg = tr.evaluate_full(x, y), tr.evaluate_full(x, y, ema=True)
    assert rep.n == N_MLP and avg.n == N_MLP and rep.bad == 0 and rep.k == 5
    assert tr.evaluate_full(x, y) == rep  # identical from call to call
    torch.cuda.synchronize()
    for n in names:
        assert torch.equal(before[n], getattr(tr, n)) and getattr(tr, n).data_ptr() == ptrs[n], n
    assert tr.graph is not None and tr.graph_unrolled is not None
    # against the definition, on the engine's own logits and loss rows of the padded set
    xp, yp = torch.zeros(256, D_IN, dtype=torch.uint8), torch.zeros(256, dtype=torch.uint8)
    xp[:N_MLP], yp[:N_MLP] = x, y
    for ema, got in ((False, rep), (True, avg)):
        logits, loss = _rows_launch(tr, xp, yp, ema=ema)
        want = E.eval_reference(logits[:N_MLP], y, loss[:N_MLP], 10, 5)
        print(ema, got.as_dict()["loss"], got.top1, got.topk)
        assert got == want, (got.as_dict(), want.as_dict())
    assert avg != rep
    # ema=True is what a second trainer holding the average reports
    second = FusedMLPTrainer(batch=B, device=DEV, seed=8, flat=tr.ema_flat())
    assert second.evaluate_full(x, y) == avg
    # whole blocks: the count evaluate() reports as a mean
    x192, y192 = x[:192], y[:192]
    r192 = tr.evaluate_full(x192, y192, topk=1)
    assert r192.n == 192 and r192.topk == r192.top1 == round(tr.evaluate(x192, y192).accuracy * 192)
    assert tr.evaluate_full(x, y, topk=10).topk == N_MLP
    for bad in (0, 11, 2.5):
        with pytest.raises(ValueError, match="topk"):
            tr.evaluate_full(x, y, topk=bad)
    with pytest.raises(ValueError, match="empty"):
        tr.evaluate_full(x[:0], y[:0])
    with pytest.raises(ValueError, match="ema"):
        second.evaluate_full(x, y, ema=True)
    tr.drop_graphs()


def test_mlp_w1_overflow_makes_every_row_bad():
    from serverless_learn_amd.models import mlp as M

    flat = M.init_params(0)
    M.views(flat)["fc1.weight"][7, 0] = 1.0e5  # beyond fp16: the update kernel flags the row sum
    tr = M.FusedMLPTrainer(batch=64, device=DEV, flat=flat)
    assert tr.w1_out_of_range()
    x, y = _mnist(70, 4)
    rep = tr.evaluate_full(x, y)
    assert (rep.n, rep.bad, rep.top1, rep.topk, rep.loss_fix) == (70, 70, 0, 0, 0) and rep.loss != rep.loss
    assert int(rep.confusion.sum()) == 0


# ---- 3. the ResNet engine, in one deterministic-build child ----
@pytest.fixture(scope="module")
def resnet_child():
    env = dict(os.environ, SL_DETERMINISTIC="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_resnet_det.py")], env=env,
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["deterministic_build"] and r["captured"], r
    return r


def test_resnet_evaluate_full_equals_the_definition(resnet_child):
    r = resnet_child["report"]
    print(r)
    assert r["n"] == r["N"] == 2 * 32 + 7, r
    assert r["equals_reference"] and r["topk1_equals_reference"] and r["second_call_identical"], r
    assert r["topk1_is_top1"] and r["cache_reused"] and r["confusion_sum"] == r["good"], r
    assert r["padding_rows_nonzero_logits"], r  # the padded rows went through the forward pass, uncounted


def test_resnet_evaluate_full_leaves_training_alone_and_the_graph_replays(resnet_child):
    s, g = resnet_child["state"], resnet_child["graph"]
    print(s, g)
    assert s["changed"] == [] and s["tensors"] > 60 and s["no_tensor_moved"], s
    assert s["shard_and_cursor_restored"] and s["graph_kept"], s
    assert g["changed_vs_twin"] == [] and g["cursor"] == 7, g


def test_resnet_evaluate_full_of_the_average_and_refusals(resnet_child):
    e, f = resnet_child["ema"], resnet_child["refusals"]
    print(e, f)
    assert e["equals_second_engine"] and e["n"] == 71 and e["differs_from_live"] and e["first_differs_from_live"], e
    assert f == {"topk0": True, "topk11": True, "empty": True, "ema_without_ema": True}, f
