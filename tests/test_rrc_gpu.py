"""input_rrc_kernel (csrc/kernels/input_rrc.hip) and the ResNet engine's augment="rrc-flip" against their
definition, serverless_learn_amd/data/augment.py rrc_params / rrc_apply: every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from serverless_learn_amd.data import augment as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 9 + (1 << 32)
# (O, batch, records, t, min_scale, shuffle).  4: one quad a row; 8, 12: one partial band (12: quantised
# weights too); 32: two bands; 64: four bands, where band seams and the 18-row bound can go wrong;
# 224, 256: the ImageNet stem's size and the largest, a whole LDS image, one source row a thread
CASES = [(4, 2, 2, 0, 0.5, False), (8, 3, 7, 1, 0.08, False), (12, 5, 11, 3, 0.08, True),
         (32, 4, 9, 2_000_000_011, 0.25, True), (64, 8, 20, 6, 0.08, True), (224, 2, 3, 5, 0.08, True),
         (256, 2, 2, 4, 0.08, False)]


def _check(O, batch, records, t, shuffle, table):
    """One launch over a seeded random shard against the definition; returns (shard, staging batch, rows)."""
    from serverless_learn_amd.ops import cnn as K

    rng = np.random.default_rng(O + records)
    x = rng.integers(0, 256, size=(records, O, O, 3), dtype=np.uint8)
    y = rng.integers(0, 10, size=records, dtype=np.uint8)
    xd, yd, tab = (torch.from_numpy(np.array(v)).to(DEV) for v in (x, y, table))
    out = torch.full((batch, O, O, 3), 7, dtype=torch.uint8, device=DEV)
    lab = torch.full((batch,), 255, dtype=torch.uint8, device=DEV)
    params, rrc = (torch.full((batch, c), -1, dtype=torch.int32, device=DEV) for c in (4, 8))
    cursor = torch.full((1,), t, dtype=torch.int32, device=DEV)
    K.input_rrc(xd, yd, cursor, batch, out, lab, params, rrc, tab, seed=SEED, shuffle=shuffle)
    torch.cuda.synchronize()
    want_p = A.rrc_params(SEED, t, records, batch, O, shuffle, table)
    assert np.array_equal(rrc.cpu().numpy(), want_p) and np.array_equal(params.cpu().numpy(), want_p[:, [0, 1, 2, 5]])
    assert np.array_equal(lab.cpu().numpy(), y[want_p[:, 0]])
    got, want = out.cpu().numpy(), A.rrc_apply(x, want_p)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (O, t, len(bad), bad[:4], want_p[bad[0][0]], got[tuple(bad[0])], want[tuple(bad[0])])
    return x, got, want_p


@pytest.mark.parametrize("O,batch,records,t,min_scale,shuffle", CASES)
def test_kernel_equals_the_definition(O, batch, records, t, min_scale, shuffle):
    _check(O, batch, records, t, shuffle, A.rrc_table(O, min_scale))


@pytest.mark.parametrize("O", (12, 64))
@pytest.mark.parametrize("box", ("reject", "1x1", "Ox1", "1xO", "too-large"))
def test_forced_tables(box, O):
    w, h = {"reject": (0, 0), "1x1": (1, 1), "Ox1": (O, 1), "1xO": (1, O), "too-large": (O + 1, O)}[box]
    x, got, p = _check(O, 6, 6, 2, True, np.full((256, 256), w | h << 16, np.int32))
    miss = box in ("reject", "too-large")  # ten misses: the whole image, or its mirror
    assert (p[:, 3:5] == ((O, O) if miss else (h, w))).all() and (p[:, 6:] == ((10, 1) if miss else (1, 0))).all()
    if miss or box == "1x1":  # (1x1: every output pixel is the one source pixel)
        want = x[p[:, 0]] if miss else x[p[:, 0], p[:, 1], p[:, 2]][:, None, None]
        unflip = np.where(p[:, 5].reshape(-1, 1, 1, 1) == 1, got[:, :, ::-1], got)
        assert set(p[:, 5]) == {0, 1} and np.array_equal(unflip, np.broadcast_to(want, got.shape))


def test_launcher_refusals():
    from serverless_learn_amd.ops import _native as N

    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)  # (never read: every call below is refused before a launch)
    ok = dict(n=4, batch=4, H=8, W=8, ptr=a)
    for bad in (dict(H=8, W=12), dict(H=10, W=10), dict(H=0, W=0), dict(H=260, W=260), dict(ptr=None), dict(n=3)):
        k = dict(ok, **bad)
        rc = N.lib().sl_input_rrc(k["ptr"], a, a, k["n"], k["batch"], k["H"], k["W"], 1, 0, a, a, a, a, a, None)
        assert rc != 0, bad


# ---- the engine ----
N_REC, BATCH, ESEED = 101, 32, 2
MIX = dict(auto_augment="trivial-wide", mixup_alpha=0.4, cutmix_alpha=1.0, label_smoothing=0.1)


def _trainer(**kw):
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    tr = FusedResNetTrainer(batch=BATCH, device=DEV, seed=ESEED, **kw)
    x, y = make_cifar_like(N_REC, seed=5)
    tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
    return tr, x, y


@pytest.mark.parametrize("kw", [{}, MIX], ids=["alone", "trivial-wide-mix"])
def test_engine_feeds_the_definition(kw):
    from serverless_learn_amd.models.resnet import CIFAR_MEAN, CIFAR_STD

    tr, x, y = _trainer(augment="rrc-flip", shuffle=True, rrc_min_scale=0.25, **kw)
    table = A.rrc_table(32, 0.25)
    for t in range(4):  # nb = 3: into epoch 1
        tr.step()
        torch.cuda.synchronize()
        params = A.rrc_params(ESEED, t, N_REC, BATCH, 32, True, table)
        assert np.array_equal(tr.rrc_out.cpu().numpy(), params), t
        assert np.array_equal(tr.aug_out.cpu().numpy(), params[:, [0, 1, 2, 5]]), t
        assert np.array_equal(tr.labels.cpu().numpy(), y[params[:, 0]]), t
        v = A.rrc_apply(x, params)
        assert np.array_equal(tr.rrc_x.cpu().numpy(), v), t
        want, cur, lab = torch.zeros_like(tr.x0), tr.cursor - 1, tr.labels.clone()
        if kw:  # TrivialAugment over the RRC batch, then the mix: the numpy definitions composed
            ta = A.ta_params(ESEED, t, BATCH)
            v = A.ta_apply(v, ta)
            assert np.array_equal(tr.ta_out.cpu().numpy(), ta) and np.array_equal(tr.ta_x.cpu().numpy(), v), t
            assert np.array_equal(tr.mix_out.cpu().numpy(), A.mix_params(ESEED, t, BATCH, 32, 32, 0.4, 1.0)), t
            tr.K.input_mix(torch.from_numpy(v).to(DEV), lab, cur, BATCH, want, lab.clone(), None, tr.mix_out.clone(),
                           tr.mix_tab, CIFAR_MEAN, CIFAR_STD, seed=ESEED, pad=0, mixup=True, cutmix=True)
        else:  # x0 is what the unchanged kernels make of the definition's batch
            tr.K.input_norm(torch.from_numpy(v).to(DEV), lab, cur, BATCH, want, lab.clone(), CIFAR_MEAN, CIFAR_STD)
        assert torch.equal(tr.x0.view(torch.int16), want.view(torch.int16)), t
        assert np.isfinite(tr.stats().loss), t


def test_engine_graph_replay_equals_eager_and_default_launches_no_input_rrc(monkeypatch):
    """Two eager (capture's warm-up) + four replayed steps against six eager ones at accum_steps = 2:
    the pipeline's buffers depend on the cursor alone, so they are compared bit for bit in either
    build, after every replay."""
    kw = dict(augment="rrc-flip", shuffle=True, accum_steps=2, **MIX)
    a, b = _trainer(**kw)[0], _trainer(**kw)[0]
    a.capture()
    for _ in range(2):
        b.step()
    for i in range(4):
        a.step()
        b.step()
        torch.cuda.synchronize()
        assert a.graph is not None and int(a.cursor.item()) == int(b.cursor.item()) == 2 * (i + 3)
        for name in ("rrc_out", "rrc_x", "aug_out", "ta_out", "ta_x", "mix_out", "x0", "labels"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (i, name)
    off = _trainer(shuffle=True)[0]
    assert all(getattr(off, n) is None for n in ("rrc_out", "rrc_x", "rrc_lab", "rrc_tab", "rrc_scratch"))
    assert set(a.state_extra()) == set(off.state_extra()) and len(a.buffers()) == len(off.buffers())
    kept = a.rrc_out.clone()
    monkeypatch.setattr(off.K, "input_rrc", lambda *a, **k: pytest.fail("input_rrc launched"))
    off.step()
    a.forward_eval()
    a.forward(train=False)
    torch.cuda.synchronize()
    assert torch.equal(a.rrc_out, kept)
