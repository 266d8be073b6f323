"""Classifier heads of 17..256 classes on the GPU: ``softmax_ce_wide_kernel`` (csrc/kernels/cnn_aux.hip) against a
float64 reference under the bounds tests/test_mix_gpu.py uses for the narrow kernel, ``eval_accum_wide_kernel``
(csrc/kernels/eval_metrics.hip) against ``eval_reference(wide=True)`` field for field, the ResNet engine with 100
and 256 classes against ``ref_grads``, the exact FC cases of utils/conv_exact.py, and the launches of a
ten-class trainer, which must be what they were.

The engine's evaluation and graph-replay checks compare bits between runs, so they run in one
``SL_DETERMINISTIC=1`` child process (this file's ``__main__``), as tests/test_mix_gpu.py and
tests/test_eval_gpu.py do."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from serverless_learn_amd.data import augment as A
from serverless_learn_amd.ops import evalmetrics as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _K():
    from serverless_learn_amd.ops import cnn as K

    return K


def rel(a, b):
    """The norm-wise measure of tests/test_cnn_gpu.py."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


# ---- 1. the loss kernel ----
def _mix(kind, n):
    """tests/test_mix_gpu.py ``_ce_mix`` for n rows: int32 [n, 8] as input_mix writes them, with num = 0 and
    num = den among them (n >= 5)."""
    m = np.zeros((n, 8), np.int32)
    m[:, 0] = (np.arange(n) + 5) % n
    if kind == "mixup":
        m[:, 1], m[:, 2], m[:, 3] = (np.arange(n) * 7) % 257, 256, 1
        if n >= 5:
            m[3, 1], m[4, 1] = 0, 256
    else:
        m[:, 1], m[:, 2], m[:, 3] = (np.arange(n) * 29) % 1025, 1024, 2
        if n >= 5:
            m[3, 1], m[4, 1] = 0, 1024
        m[:, 4:] = (1, 2, 3, 4)
    return m


def test_mix_rows_are_those_of_test_mix_gpu():
    from test_mix_gpu import _ce_mix

    for kind in ("mixup", "cutmix"):
        assert np.array_equal(_mix(kind, 37), _ce_mix(kind))


@functools.lru_cache(maxsize=None)
def _ce_inputs(n, ncls):
    g = torch.Generator().manual_seed(1000 * ncls + n)
    z = torch.randn(n, ncls, generator=g) * 3
    lab = torch.randint(0, ncls, (n,), generator=g, dtype=torch.uint8)
    if n >= 3:
        z[1, 3] = z[1, ncls - 1] = 11.0  # the maximum twice: the lowest index wins,
        lab[1] = ncls - 1                # so this row is not correct
        if ncls < 256:
            lab[2] = ncls                # a label >= ncls counts as 0
    return z.to(DEV), lab.to(DEV)


def _ce_run(fn, z, lab, ldd=None, ws="make", db0=0.0, **kw):
    K = _K()
    n, ncls = z.shape
    ldd = K.logit_ld(ncls) if ldd is None else ldd
    loss = torch.full((n,), 9.0, device=DEV)
    corr = torch.full((n,), 9.0, device=DEV)
    dz = torch.full((n, ldd), 9.0, dtype=torch.bfloat16, device=DEV)
    db = torch.full((ncls,), db0, device=DEV)
    if isinstance(ws, str):
        ws = K.softmax_ce_wide_ws(n, ncls, DEV)
        ws.fill_(NAN)  # it holds nothing between calls
    try:
        fn(z, lab, loss, corr, dz, db, 0.5, ws=ws, **kw)
    finally:
        torch.cuda.synchronize()
    return loss, corr, dz, db


SHAPES = [(37, 17), (37, 64), (37, 65), (37, 100), (37, 255), (37, 256), (1, 100), (1030, 100)]


@pytest.mark.parametrize("n,ncls", SHAPES)
def test_wide_loss_against_float64(n, ncls):
    K = _K()
    z, lab = _ce_inputs(n, ncls)
    ldd = K.logit_ld(ncls)
    assert ldd == max(32, 1 << (ncls - 1).bit_length())
    lab_c = np.where(lab.cpu().numpy() < ncls, lab.cpu().numpy(), 0)
    own = torch.from_numpy(lab_c).long()
    want_corr = (z.cpu().argmax(1) == own).float()
    if n >= 3:
        assert want_corr[1] == 0
    forms = [("one-hot", K.softmax_ce, {}, None, 0.0)]
    for eps in (0.0, 0.1):
        for kind in (None, "mixup", "cutmix"):
            m = None if kind is None else _mix(kind, n)
            kw = dict(mix=None if m is None else torch.from_numpy(m).to(DEV), eps=eps)
            forms.append((f"soft eps {eps} mix {kind}", K.softmax_ce_soft, kw, m, eps))
    for name, fn, kw, m, eps in forms:
        loss, corr, dz, db = _ce_run(fn, z, lab, **kw)
        q = torch.from_numpy(A.soft_targets(lab_c, m, eps, ncls))
        assert float((q.sum(1) - 1).abs().max()) < 1e-12
        zr = z.double().cpu().requires_grad_(True)
        want = torch.logsumexp(zr, 1) - (q * zr).sum(1)
        (want.sum() * 0.5).backward()
        figs = (rel(loss, want), rel(dz[:, :ncls], zr.grad), rel(db, zr.grad.sum(0)))
        print(f"{n}x{ncls} {name}: loss rel {figs[0]:.2e} dz rel {figs[1]:.2e} dbias rel {figs[2]:.2e}")
        assert figs[0] < 1e-4, (name, figs)
        assert figs[1] < 1e-2, (name, figs)
        assert figs[2] < 1e-4, (name, figs)
        assert dz.shape[1] == ldd and (ldd == ncls or int((_bits(dz[:, ncls:]) != 0).sum()) == 0), name
        assert torch.equal(corr.cpu(), want_corr), name
        # the same bits from call to call, all four outputs (onto a non-zero dbias too)
        again = _ce_run(fn, z, lab, **kw)
        for a, b in zip((loss, corr, dz, db), again):
            assert torch.equal(_bits(a), _bits(b)), name
        a, b = _ce_run(fn, z, lab, db0=0.75, **kw), _ce_run(fn, z, lab, db0=0.75, **kw)
        assert torch.equal(_bits(a[3]), _bits(b[3])) and not torch.equal(a[3], db)
    hard = _ce_run(K.softmax_ce, z, lab)
    soft = _ce_run(K.softmax_ce_soft, z, lab, mix=None, eps=0.0)
    for a, b in zip(hard, soft):  # the soft form at eps = 0 without a mix: the one-hot form, bit for bit
        assert torch.equal(_bits(a), _bits(b))


def test_wide_loss_without_a_bias_gradient_and_a_wider_stride():
    """dbias = None (the evaluation paths) leaves the workspace alone; any power-of-two stride up to 256."""
    K = _K()
    z, lab = _ce_inputs(37, 100)
    n, ncls = z.shape
    base = _ce_run(K.softmax_ce, z, lab)
    loss, corr = torch.full((n,), 9.0, device=DEV), torch.full((n,), 9.0, device=DEV)
    dz = torch.full((n, 256), 9.0, dtype=torch.bfloat16, device=DEV)
    ws = torch.full((4096,), 7.0, device=DEV)
    K.softmax_ce(z, lab, loss, corr, dz, None, 0.5, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(loss, base[0]) and torch.equal(corr, base[1])
    assert torch.equal(_bits(dz[:, :128]), _bits(base[2])) and int((_bits(dz[:, 128:]) != 0).sum()) == 0
    assert float((ws - 7.0).abs().max()) == 0


def test_wide_loss_refusals_write_nothing():
    K = _K()
    z, lab = _ce_inputs(37, 100)

    def untouched(out):
        return all(float((t.float() - 9.0).abs().max()) == 0 for t in out[:3]) and float(out[3].abs().max()) == 0

    for ldd in (64, 96, 104, 16, 512):  # below ncls, no power of two (twice), the narrow stride, above 256
        with pytest.raises(RuntimeError, match="sl_softmax_ce_wide"):
            _ce_run(K.softmax_ce, z, lab, ldd=ldd)
        with pytest.raises(RuntimeError, match="sl_softmax_ce_wide"):
            _ce_run(K.softmax_ce_soft, z, lab, ldd=ldd, eps=0.1)
    z257 = torch.zeros(37, 257, device=DEV)
    big = torch.empty(1 << 16, device=DEV)
    with pytest.raises(RuntimeError, match="sl_softmax_ce_wide"):
        _ce_run(K.softmax_ce, z257, lab, ldd=512, ws=big)
    with pytest.raises(RuntimeError, match="sl_softmax_ce_wide"):
        _ce_run(K.softmax_ce, z257, lab, ldd=256, ws=big)
    with pytest.raises(ValueError, match="workspace"):
        _ce_run(K.softmax_ce, z, lab, ws=None)
    with pytest.raises(ValueError, match="workspace"):
        _ce_run(K.softmax_ce_soft, z, lab, ws=None, eps=0.1)
    with pytest.raises(RuntimeError, match="sl_softmax_ce_wide"):  # a workspace shorter than the partial rows
        _ce_run(K.softmax_ce, z, lab, ws=torch.empty(128, device=DEV))
    with pytest.raises(ValueError, match="smoothing"):
        _ce_run(K.softmax_ce_soft, z, lab, eps=1.0)
    # nothing was launched by any of them: the same buffers, passed by hand
    n, ncls = z.shape
    out = (torch.full((n,), 9.0, device=DEV), torch.full((n,), 9.0, device=DEV),
           torch.full((n, 64), 9.0, dtype=torch.bfloat16, device=DEV), torch.zeros(ncls, device=DEV))
    ws = K.softmax_ce_wide_ws(n, ncls, DEV)
    with pytest.raises(RuntimeError):
        K.softmax_ce(z, lab, out[0], out[1], out[2], out[3], 0.5, ws=ws)
    with pytest.raises(ValueError):
        K.softmax_ce(z, lab, out[0], out[1], out[2].new_full((n, 128), 9.0), out[3], 0.5)
    with pytest.raises(RuntimeError):
        K.softmax_ce(z, lab, out[0], out[1], out[2].new_full((n, 128), 9.0), out[3], 0.5, ws=ws[:100])
    torch.cuda.synchronize()
    assert untouched(out)
    assert K.softmax_ce_wide_ws(37, 10, DEV) is None
    for bad in (0, 257, 2.5):
        with pytest.raises(ValueError, match="classes"):
            K.logit_ld(bad)
    assert [K.logit_ld(c) for c in (1, 10, 16, 17, 32, 33, 100, 128, 129, 256)] == [16, 16, 16, 32, 32, 64, 128, 128, 256, 256]


# ---- 2. the evaluation kernel ----
ROWS = 203  # 6 whole workgroups of 32 rows, one whole wave of 8 and a wave with 3


def _block(rep: E.EvalReport) -> np.ndarray:
    ncls = rep.confusion.shape[0]
    a = np.zeros(E.acc_len_wide(ncls), np.int64)
    a[:5] = (rep.n, rep.bad, rep.top1, rep.topk, rep.loss_fix)
    a[E.ACC_HEAD:] = rep.confusion.reshape(-1)
    return a


def _case(rows: int, ncls: int, seed: int = 0):
    """tests/test_eval_gpu.py ``_case`` over ncls classes: logits from the integer grid -2..2 (ties are
    frequent), arbitrary positive losses and the same planted rows."""
    g = torch.Generator().manual_seed(seed + 131 * ncls + rows)
    z = torch.randint(-2, 3, (rows, ncls), generator=g).float()
    lab = torch.randint(0, ncls, (rows,), generator=g).to(torch.uint8)
    loss = (torch.rand(rows, generator=g) * 5).float()
    z[0] = 0.0
    z[0, 0] = z[0, 2] = 3.0
    lab[0] = 2                   # the maximum ties include the label, at a higher index: pred 0, rank 1
    z[1] = 0.0
    z[1, 1] = z[1, ncls - 1] = 3.0
    lab[1] = 1                   # ... at the lowest index: pred 1, rank 0
    z[2, 3] = NAN                # bad rows: a NaN logit,
    z[3, ncls - 1] = INF         # a +inf logit in the last class,
    loss[4] = NAN                # a NaN loss,
    loss[5] = 65536.0            # a loss of exactly 2^16
    loss[6] = -1e-7              # a tiny negative loss: good, rounds to -2 units
    if ncls < 256:
        lab[7] = ncls            # a label >= ncls counts as 0 (a u8 cannot reach 256)
    loss[17] = 65535.996         # the largest fp32 below 2^16: good
    z[40, 1] = -INF              # bad rows in the later waves and workgroups too
    z[100, ncls - 2] = NAN
    loss[150] = -INF
    loss[202] = -65536.0
    z[9] = -2.0
    z[9, ncls - 1] = 2.0
    lab[9] = ncls - 1            # the maximum in the last lane that holds a class
    return z, lab, loss


@pytest.fixture(scope="module")
def cases():
    return {ncls: _case(ROWS, ncls) for ncls in (17, 100, 256)}


def _launch(z, lab, loss, n_valid, ncls, topk, acc=None, ld=None):
    """The rows on the device with everything from row n_valid on poisoned (NaN logits and loss, label 255);
    the logits as a view of a [rows, ld] buffer when ``ld`` is given."""
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
    acc = E.new_acc_wide(DEV, ncls) if acc is None else acc
    E.eval_accum_wide(zd, ld_.to(DEV), lo.to(DEV), n_valid, ncls, topk, acc)
    return acc


@pytest.mark.parametrize("n_valid", [203, 1, 0])
@pytest.mark.parametrize("topk", [1, 5, "ncls"])
@pytest.mark.parametrize("ncls", [17, 100, 256])
def test_wide_eval_kernel_equals_the_definition(cases, ncls, topk, n_valid):
    topk = ncls if topk == "ncls" else topk
    z, lab, loss = cases[ncls]
    want = E.eval_reference(z[:n_valid], lab[:n_valid], loss[:n_valid], ncls, topk, wide=True)
    acc = _launch(z, lab, loss, n_valid, ncls, topk)
    got = acc.cpu().numpy()
    print(ncls, topk, n_valid, got[:8], want.as_dict()["loss"])
    assert got.shape == (8 + ncls * ncls,) and np.array_equal(got, _block(want)), (got[:8], _block(want)[:8])
    assert E.report_from_acc_wide(acc, ncls, topk) == want
    if n_valid == ROWS:  # every planted row took part
        assert want.bad == 8 and want.n == ROWS and int(want.confusion.sum()) == ROWS - 8
        assert want.confusion[2, 0] >= 1 and want.confusion[1, 1] >= 1 and want.confusion[ncls - 1, ncls - 1] >= 1
        assert (want.topk == want.top1) if topk == 1 else (want.topk > want.top1)
        assert (want.topk == want.n - want.bad) if topk == ncls else True
    # adds, never overwrites: a second launch without zeroing doubles every field
    _launch(z, lab, loss, n_valid, ncls, topk, acc=acc)
    assert np.array_equal(acc.cpu().numpy(), 2 * _block(want))
    # the row stride is an argument: the same rows inside wider buffers whose other columns are NaN
    for ld in (ncls + 3, 260):  # rows on 4-byte boundaries only; rows on 16-byte boundaries
        assert np.array_equal(_launch(z, lab, loss, n_valid, ncls, topk, ld=ld).cpu().numpy(), _block(want)), ld


def test_wide_eval_entry_point_refuses_bad_arguments():
    z, lab, loss = (t.to(DEV) for t in _case(ROWS, 100))
    acc = E.new_acc_wide(DEV, 100)
    for kw in (dict(ncls=257), dict(ncls=0), dict(topk=0), dict(topk=101), dict(n_valid=204), dict(n_valid=-1)):
        a = dict(n_valid=ROWS, ncls=100, topk=5)
        a.update(kw)
        big = torch.zeros(8 + 257 * 257, dtype=torch.int64, device=DEV)
        with pytest.raises((RuntimeError, ValueError), match="sl_eval_accum_wide|ncls"):
            E.eval_accum_wide(z, lab, loss, a["n_valid"], a["ncls"], a["topk"], big)
        assert int(big.abs().sum()) == 0
    with pytest.raises(RuntimeError, match="sl_eval_accum_wide"):  # a row stride shorter than the classes
        E.eval_accum_wide(z[:, :60].contiguous(), lab, loss, ROWS, 100, 5, acc)
    with pytest.raises(ValueError):  # the narrow block is too short for 100 classes
        E.eval_accum_wide(z, lab, loss, ROWS, 100, 5, E.new_acc(DEV))
    with pytest.raises(TypeError):
        E.eval_accum_wide(z.double(), lab, loss, ROWS, 100, 5, acc)
    with pytest.raises(RuntimeError, match="sl_eval_accum"):  # the narrow entry point is what it was
        E.eval_accum(z[:, :17].contiguous(), lab, loss, ROWS, 17, 5, E.new_acc(DEV))
    assert int(acc.abs().sum()) == 0  # nothing was launched


# ---- 3. the engine ----
def _engine(stem, batch, hw, classes, seed=3, **kw):
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    tr = FusedResNetTrainer(batch=batch, device=DEV, stem=stem, classes=classes, momentum=0.0, weight_decay=0.0,
                            in_hw=hw, **kw)
    x, y = make_cifar_like(batch, seed=seed, hw=hw, classes=classes)
    tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
    return tr, x, y


@pytest.mark.parametrize("stem,batch,hw,classes", [("cifar", 32, 32, 100), ("imagenet", 8, 64, 256)])
def test_engine_grads_match_reference(stem, batch, hw, classes):
    """tests/test_cnn_gpu.py test_resnet_engine_grads_match_reference with a wide head, under its bounds."""
    from serverless_learn_amd.models.resnet import ref_grads, running_stats

    tr, x, y = _engine(stem, batch, hw, classes)
    assert tr.logit_ld == (128 if classes == 100 else 256) and tr.wide and tr.ce_ws is not None
    assert tr.dlogits.shape == (batch, 1, 1, tr.logit_ld) and tr.fc_wt.numel() == 512 * tr.logit_ld
    g = tr.compute_grads().clone()
    torch.cuda.synchronize()
    assert int(y.max()) > 16
    loss_ref, corr_ref, g_ref = ref_grads(tr.spec, tr.params.detach().clone(), torch.from_numpy(x).to(DEV),
                                          torch.from_numpy(y).to(DEV), 1.0 / batch, running_stats(tr.spec, DEV))
    loss = float(tr.loss.sum())
    print(stem, classes, "loss", loss, float(loss_ref))
    assert abs(loss - float(loss_ref)) / float(loss_ref) < 0.03, (loss, float(loss_ref))
    spec = tr.spec
    bad = []
    for c in spec.convs():
        cos = float(F.cosine_similarity(g[c.off:c.off + c.numel], g_ref[c.off:c.off + c.numel], dim=0))
        if cos < 0.85:
            bad.append((c.name, cos))
    for bn in spec.bns():
        a = torch.cat([g[bn.g_off:bn.g_off + bn.c], g[bn.b_off:bn.b_off + bn.c]])
        b = torch.cat([g_ref[bn.g_off:bn.g_off + bn.c], g_ref[bn.b_off:bn.b_off + bn.c]])
        cos = float(F.cosine_similarity(a, b, dim=0))
        if cos < 0.85:
            bad.append((bn.name, cos))
    fc = slice(spec.fc_w, spec.fc_w + spec.classes * 512)
    cw = float(F.cosine_similarity(g[fc], g_ref[fc], dim=0))
    print("fc cos", cw, "below 0.85:", bad)
    assert cw > 0.99
    assert not bad, bad
    # the bias gradient against float64 on the engine's own logits, under the kernel's own bound
    zr = tr.logits.double().cpu().requires_grad_(True)
    (F.cross_entropy(zr, torch.from_numpy(y).long(), reduction="sum") / batch).backward()
    db = rel(g[spec.fc_b:spec.fc_b + classes], zr.grad.sum(0))
    print("fc bias gradient rel", db)
    assert db < 1e-4, db
    assert int((_bits(tr.dlogits.view(batch, tr.logit_ld)[:, classes:]) != 0).sum()) == 0


def test_engine_refuses_classes_out_of_range():
    from serverless_learn_amd.models.resnet_engine import LOGIT_LD, FusedResNetTrainer

    for bad in (0, 257, -3, 2.5):
        with pytest.raises(ValueError, match="classes"):
            FusedResNetTrainer(batch=8, device=DEV, classes=bad)
    assert LOGIT_LD == 16


@pytest.fixture(scope="module")
def det_child():
    env = dict(os.environ, SL_DETERMINISTIC="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=280)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["deterministic_build"], r
    return r


def test_engine_evaluate_full_equals_the_definition(det_child):
    for key in ("live", "ema"):
        r = det_child["eval"][key]
        print(key, r)
        assert r["n"] == 70 and r["equals_reference"] and r["confusion_shape"] == [100, 100], r
        assert r["confusion_sum"] == r["n"] - r["bad"] and r["second_call_identical"], r
    assert det_child["eval"]["ema_differs_from_live"]
    s = det_child["eval"]["state"]
    assert s["changed"] == [] and s["tensors"] > 60 and s["no_tensor_moved"] and s["cursor"] == s["cursor_before"], s


def test_engine_captured_step_replays_to_the_eager_parameters(det_child):
    for key in ("one_hot", "soft"):
        r = det_child["graph"][key]
        print(key, r)
        assert r["captured"] and r["changed_vs_eager"] == [] and r["cursor"] == 5 and r["finite"], r


def _child():
    """The engine's bit-exact checks with 100 classes (SL_DETERMINISTIC=1): one JSON line."""
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    K = _K()
    B, NCLS, N = 32, 100, 70
    x, y = (torch.from_numpy(a) for a in make_cifar_like(4 * B, seed=5, classes=NCLS))
    xe, ye = (torch.from_numpy(a) for a in make_cifar_like(N, seed=6, classes=NCLS))
    ye[3] = 200  # a label >= classes counts as 0

    def trainer(**kw):
        tr = FusedResNetTrainer(batch=B, device=DEV, seed=2, classes=NCLS, in_hw=32, **kw)
        tr.load_shard(x, y)
        return tr

    def state(tr):
        d = {"params": tr.params, "shadow": tr.shadow, "mom": tr.mom, "ema": tr.ema, "ema_step": tr.ema_step,
             "cursor": tr.cursor, "fc_wt": tr.fc_wt, "grad": tr.grad}
        d.update({f"wt/{name}": c.wt for name, c in tr.conv.items()})
        for name, (rm, rv) in tr.running_stats().items():
            d[f"bn/{name}/mean"], d[f"bn/{name}/var"] = rm, rv
        return {k: v for k, v in d.items() if v is not None}

    def same(a, b):
        return sorted(k for k in a if not torch.equal(a[k], b[k]))

    out = {"deterministic_build": K.deterministic(), "graph": {}}
    # a captured step against eager steps: two eager + three replays, against five eager
    for key, kw in (("one_hot", {}), ("soft", dict(label_smoothing=0.1, mixup_alpha=0.4, cutmix_alpha=1.0))):
        a, b = trainer(**kw), trainer(**kw)
        a.capture(warmup=2)
        for _ in range(3):
            a.step()
        for _ in range(5):
            b.step()
        torch.cuda.synchronize()
        out["graph"][key] = {"captured": a.graph is not None and b.graph is None,
                             "changed_vs_eager": same(state(a), state(b)), "cursor": int(a.cursor.item()),
                             "finite": bool(torch.isfinite(a.params).all()) and bool(np.isfinite(a.stats().loss))}
        a.drop_graphs()
    # evaluate_full over 70 records (two whole batches and a tail of 6) against the definition applied to
    # the trainer's own logits and loss rows
    tr = trainer(ema_decay=0.5)
    for _ in range(3):
        tr.step()
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in state(tr).items()}
    ptrs = {k: v.data_ptr() for k, v in state(tr).items()}
    reps = {False: tr.evaluate_full(xe, ye, topk=5), True: tr.evaluate_full(xe, ye, ema=True, topk=5)}
    again = {False: tr.evaluate_full(xe, ye, topk=5), True: tr.evaluate_full(xe, ye, ema=True, topk=5)}
    torch.cuda.synchronize()
    after = state(tr)
    ev = {"state": {"changed": same(before, after), "tensors": len(before), "cursor_before": int(before["cursor"].item()),
                    "no_tensor_moved": all(after[k].data_ptr() == p for k, p in ptrs.items()),
                    "cursor": int(tr.cursor.item())},
          "ema_differs_from_live": bool(reps[True] != reps[False])}
    rows = (N + B - 1) // B * B
    xp = torch.zeros(rows, 32, 32, 3, dtype=torch.uint8, device=DEV)
    yp = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    xp[:N].copy_(xe.reshape(N, 32, 32, 3))
    yp[:N].copy_(ye)
    for ema in (False, True):
        if ema:
            tr.set_flat(tr.ema_flat())  # (after the state comparison: the live weights are no longer needed)
        saved = (tr.x, tr.y, tr.cursor)
        tr.x, tr.y, tr.cursor = xp, yp, torch.zeros(1, dtype=torch.int32, device=DEV)
        logits, loss = [], []
        for _ in range(rows // B):
            tr.forward_eval()
            logits.append(tr.logits.clone())
            loss.append(tr.loss.clone())
            K.cursor_bump(tr.cursor)
        tr.x, tr.y, tr.cursor = saved
        logits, loss = torch.cat(logits).cpu(), torch.cat(loss).cpu()
        want = E.eval_reference(logits[:N], ye, loss[:N], NCLS, 5, wide=True)
        rep = reps[ema]
        ev["ema" if ema else "live"] = {
            "n": rep.n, "bad": rep.bad, "equals_reference": bool(rep == want), "confusion_shape": list(rep.confusion.shape),
            "confusion_sum": int(rep.confusion.sum()), "second_call_identical": bool(rep == again[ema]),
            "top1": rep.top1, "topk": rep.topk, "loss": rep.loss}
    out["eval"] = ev
    print(json.dumps(out))


# ---- 4. a ten-class trainer launches what it did ----
class _Recorder:
    """Stands in for the loaded kernel library: every ``sl_*`` call is logged as (name, the arguments that are
    not pointers) and passed on."""

    def __init__(self, lib, sigs, log):
        self._lib, self._sigs, self._log = lib, sigs, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("sl_"):
            return fn
        import ctypes

        types = self._sigs.get(name, [])

        def call(*a):
            self._log.append((name, tuple(v for v, t in zip(a, types) if t is not ctypes.c_void_p)))
            return fn(*a)

        return call


def record_launches(classes=None):
    """(name, scalars) of every native call of a ten-class trainer's second eager step, an eval-mode
    forward and a held-out evaluation of 40 records (two batches, the second with 8 valid rows)."""
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer
    from serverless_learn_amd.ops import _native

    kw = {} if classes is None else dict(classes=classes)
    tr = FusedResNetTrainer(batch=32, device=DEV, seed=1, **kw)
    x, y = (torch.from_numpy(a) for a in make_cifar_like(64, seed=5))
    tr.load_shard(x, y)
    tr.step()  # (sizes the split-K slab)
    torch.cuda.synchronize()
    log, real = [], _native.lib
    lib = real()
    _native.lib = lambda: _Recorder(lib, _native._SIGS, log)
    try:
        tr.step()
        tr.forward_eval()
        tr.evaluate_full(x[:40], y[:40])
        torch.cuda.synchronize()
    finally:
        _native.lib = real
    return [(n, tuple(round(v, 9) if isinstance(v, float) else v for v in a)) for n, a in log]


def launches_digest(log):
    return hashlib.sha256(repr(log).encode()).hexdigest()


# calls per entry point, their number, and the digest of the whole ordered list with its scalar arguments,
# recorded at the commit before the wide head (the same trainer, the same three calls)
TEN_CLASS_CALLS = {
    "sl_avgpool_bwd": 1, "sl_avgpool_fwd": 4, "sl_bn_apply": 51, "sl_bn_apply_stats": 14, "sl_bn_bwd_apply_dual": 3,
    "sl_bn_bwd_apply_sums": 14, "sl_bn_bwd_reduce": 1, "sl_conv3x3_bnin_fwd": 3, "sl_conv3x3_bnin_wgrad": 3,
    "sl_conv_dgrad": 1, "sl_conv_dgrad_bnx": 16, "sl_conv_dgrad_s2_even": 3, "sl_conv_fwd": 81, "sl_conv_wgrad": 18,
    "sl_conv_wgrad_ws_need": 1, "sl_conv_wt": 1, "sl_cursor_bump": 3, "sl_eval_accum": 2, "sl_input_norm": 4,
    "sl_sgd_flat": 1, "sl_softmax_ce": 4,
}
TEN_CLASS_DIGEST = "10d1cdd8d0992cc292bf5fc34cb0c7c72ef76592ce0108cf8a82d3067392c154"


def test_a_ten_class_trainer_launches_what_it_did():
    import collections

    log = record_launches()
    assert log == record_launches(classes=10)
    calls = dict(collections.Counter(n for n, _ in log))
    print(sorted(calls.items()), len(log), launches_digest(log))
    assert not [n for n, _ in log if "wide" in n]
    assert calls == TEN_CLASS_CALLS and len(log) == 229
    # (name, dlogits stride, classes) of the loss launches and the FC's three GEMM calls are in the digest
    assert ("sl_softmax_ce", (16, 32, 10, 1.0 / 32)) in log
    assert launches_digest(log) == TEN_CLASS_DIGEST


# ---- 5. the exact FC cases ----
@pytest.mark.parametrize("name", ["H1-fc-37x512-100", "H2-fc-37x512-250"])
def test_fc_exact_cases(name):
    from serverless_learn_amd.utils import conv_exact as X

    case = {c.name: c for c in X.FC_CASES}[name]
    K = _K()
    assert case.bias and case.do_dgrad and case.ldd == K.logit_ld(case.shape[4]) and case.fwd and case.dgrad and case.wgrad
    assert not set(c.name for c in X.FC_CASES) & set(X.CASES_BY_NAME)
    r = X.run_case(case, DEV, keep=True)
    print(r["seen"], r["maxima"])
    assert r["failures"] == [], "\n".join(r["failures"])
    # run_case compares with torch.equal; once more here, on what it kept
    o = X.operands(case, DEV)
    ref = X.case_reference(case, o)
    assert torch.equal(r["out"]["y"].double(), ref["y"]) and torch.equal(r["out"]["dx_add"].double(), ref["dx_add"])
    assert torch.equal(r["out"]["dw"].double(), ref["dw"])
    assert set(case.fwd) <= set(r["seen"]["fwd"]) and set(case.dgrad) <= set(r["seen"]["dgrad"])
    assert all(set(case.wgrad) <= set(r["seen"]["wgrad[%d]" % t]) for t in case.target_wgs)


if __name__ == "__main__":  # the child process of det_child
    _child()
