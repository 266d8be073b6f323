"""input_ta_kernel (csrc/kernels/input_ta.hip) and the ResNet engine's auto_augment="trivial-wide"
against their definition, serverless_learn_amd/data/augment.py ta_apply: every comparison is exact.
The engine's x0 is compared as tests/test_mix_gpu.py does: the definition's batch in pixel units,
normalised in float64 (where the product and the sum are exact) and rounded once to fp32, then bf16."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from serverless_learn_amd.data import augment as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(3, 8, 8), (2, 12, 20), (5, 32, 32), (2, 64, 64), (2, 5, 7)]  # (5, 7): 105 bytes, the byte-wise stream


@functools.lru_cache(maxsize=None)
def _shard(b, h, w):
    """2 b records, so cursors 0 and 1 are one epoch and draw every record once: seeded random images
    and, in turn, a constant one, a two-level one (Equalize's step == 0) and one with a constant
    channel (AutoContrast's hi == lo).  (x, y) on the host, then x, y and ta_table() on the device."""
    rng = np.random.default_rng(100 * h + w)
    x = rng.integers(0, 256, size=(2 * b, h, w, 3), dtype=np.uint8)
    x[1::4] = 93
    x[2::4] = np.where(np.arange(h * w).reshape(h, w, 1) % 32 == 0, 40, 200)
    x[3::4, :, :, 1] = 17
    y = rng.integers(0, 10, size=2 * b, dtype=np.uint8)
    x.setflags(write=False)
    return (x, y) + tuple(torch.from_numpy(v.copy()).to(DEV) for v in (x, y, A.ta_table()))


def _check(shape, t, ta_rows, force, seed=5):
    from serverless_learn_amd.ops import cnn as K

    b, h, w = shape
    pad = min(4, h - 1)
    x, y, xd, yd, tab = _shard(*shape)
    params = A.batch_params(seed, t, 2 * b, b, pad, True, "crop-flip")
    want = A.ta_apply(A.apply(x, params, pad), ta_rows)
    out = torch.full((b, h, w, 3), 7, dtype=torch.uint8, device=DEV)
    lab = torch.full((b,), 255, dtype=torch.uint8, device=DEV)
    got_p, got_ta = (torch.full((b, 4), -1, dtype=torch.int32, device=DEV) for _ in range(2))
    cursor = torch.full((1,), t, dtype=torch.int32, device=DEV)
    K.input_ta(xd, yd, cursor, b, out, lab, got_p, got_ta, tab, seed=seed, shuffle=True, augment="crop-flip", pad=pad,
               force=force)
    torch.cuda.synchronize()
    assert np.array_equal(got_p.cpu().numpy(), params) and np.array_equal(got_ta.cpu().numpy(), ta_rows)
    assert np.array_equal(lab.cpu().numpy(), y[params[:, 0]])
    got = out.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (shape, t, ta_rows[0], len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("bin_neg", [(0, 0), (30, 0), (30, 1), (17, 1)])
@pytest.mark.parametrize("op", range(14))
def test_kernel_equals_the_definition(op, bin_neg, shape):
    rows = np.tile(np.array([op, *bin_neg, 0], np.int32), (shape[0], 1))
    for t in (0, 1):
        _check(shape, t, rows, op | bin_neg[0] << 8 | bin_neg[1] << 16)


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_draws_as_the_definition(shape):
    for t in (0, 1, 2_000_000_011):
        _check(shape, t, A.ta_params(9 + (1 << 32), t, shape[0]), -1, seed=9 + (1 << 32))


# ---- the engine ----
N_REC, BATCH, SEED = 101, 32, 2
PIPE = dict(augment="crop-flip", shuffle=True)
MIX = dict(PIPE, mixup_alpha=0.4, cutmix_alpha=1.0, label_smoothing=0.1)


def _cifar():
    from serverless_learn_amd.data.synthetic import make_cifar_like

    return make_cifar_like(N_REC, seed=5)


def _trainer(**kw):
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    tr = FusedResNetTrainer(batch=BATCH, device=DEV, seed=SEED, **kw)
    tr.load_shard(*(torch.from_numpy(v) for v in _cifar()))
    return tr


def _norm_bits(v):
    """bf16 bits [B,H,W,8] (int16, on the host) of pixel-unit values v [B,H,W,3] (tests/test_mix_gpu.py)."""
    from serverless_learn_amd.models.resnet import CIFAR_MEAN, CIFAR_STD

    m, s = np.asarray(CIFAR_MEAN, np.float32), np.asarray(CIFAR_STD, np.float32)
    a = (np.float32(1) / (np.float32(255) * s)).astype(np.float32)  # the launcher's fp32 arithmetic
    b = (-m / s).astype(np.float32)
    f = (v.astype(np.float64) * a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
    out = torch.zeros(*v.shape[:3], 8, dtype=torch.bfloat16)
    out[..., :3] = torch.from_numpy(f).to(torch.bfloat16)
    return out.view(torch.int16)


@pytest.mark.parametrize("kw", [{}, PIPE, MIX], ids=["alone", "crop-flip-shuffle", "mix"])
def test_engine_feeds_the_definition(kw):
    tr = _trainer(auto_augment="trivial-wide", **kw)
    x, y = _cifar()
    assert tuple(tr.ta_out.shape) == (BATCH, 4) and tr.ta_out.dtype == torch.int32
    for t in range(4):  # nb = 3: into epoch 1
        tr.step()
        torch.cuda.synchronize()
        params = A.batch_params(SEED, t, N_REC, BATCH, 4, kw.get("shuffle", False), kw.get("augment", "none"))
        ta = A.ta_params(SEED, t, BATCH)
        v = A.ta_apply(A.apply(x, params, 4), ta)
        assert np.array_equal(tr.aug_out.cpu().numpy(), params) and np.array_equal(tr.ta_out.cpu().numpy(), ta), t
        assert np.array_equal(tr.labels.cpu().numpy(), y[params[:, 0]]), t
        if "mixup_alpha" in kw:
            mix = A.mix_params(SEED, t, BATCH, 32, 32, 0.4, 1.0)
            assert np.array_equal(tr.mix_out.cpu().numpy(), mix), t
            v = A.mix_apply(v, mix)
        assert torch.equal(tr.x0.view(torch.int16).cpu(), _norm_bits(v.astype(np.float32))), t
        assert np.isfinite(tr.stats().loss), t


def test_engine_evaluation_and_default_launch_no_input_ta(monkeypatch):
    on, off = _trainer(auto_augment="trivial-wide", **PIPE), _trainer(**PIPE)
    assert off.ta_out is None and off.ta_x is None and off.ta_lab is None and off.ta_tab is None
    on.step()
    torch.cuda.synchronize()
    kept = on.ta_out.clone(), on.ta_x.clone()
    monkeypatch.setattr(on.K, "input_ta", lambda *a, **k: pytest.fail("input_ta launched"))
    off.step()
    x, y = _cifar()
    for fwd in (on.forward_eval, lambda: on.forward(train=False),
                lambda: on.evaluate(torch.from_numpy(x[:64].copy()), torch.from_numpy(y[:64].copy()))):
        fwd()
    torch.cuda.synchronize()
    assert torch.equal(on.ta_out, kept[0]) and torch.equal(on.ta_x, kept[1]) and int(on.cursor.item()) == 1
    assert set(on.state_extra()) == set(off.state_extra()) and len(on.buffers()) == len(off.buffers())


def _graph_checks():
    """Two eager (capture's warm-up) + three replayed steps against five eager ones, accum_steps = 2."""
    from serverless_learn_amd.ops import cnn as K

    kw = dict(auto_augment="trivial-wide", accum_steps=2, **MIX)
    a, b = _trainer(**kw), _trainer(**kw)
    a.capture()
    for _ in range(3):
        a.step()
    for _ in range(5):
        b.step()
    torch.cuda.synchronize()
    assert a.graph is not None and int(a.cursor.item()) == int(b.cursor.item()) == 10
    for name in ("params", "grad", "loss", "ta_out", "aug_out", "mix_out", "ta_x"):
        assert getattr(a, name).cpu().numpy().tobytes() == getattr(b, name).cpu().numpy().tobytes(), name
    return K.deterministic()


def test_engine_graph_replay_equals_eager_under_accumulation():
    """A process loads one kernel library: the bit comparison runs in a child process with the
    deterministic build, whose cross-workgroup sums do not depend on the order of atomics."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SL_DETERMINISTIC="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=root, capture_output=True,
                         text=True, timeout=170)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2000:])
    assert json.loads(out.stdout.strip().splitlines()[-1]) == {"deterministic_build": True, "ok": True}


if __name__ == "__main__":  # the child process of test_engine_graph_replay_equals_eager_under_accumulation
    print(json.dumps({"deterministic_build": _graph_checks(), "ok": True}))
