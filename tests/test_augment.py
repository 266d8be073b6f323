"""The input pipeline's definition (serverless_learn_amd/data/augment.py): the epoch permutation is
a bijection that really shuffles, the crop / flip draws cover their range, the off states are
today's batches, the zero-padded gather matches a hand-written loop, and the CPU trainer, the
configuration and the worker carry the three settings."""
import argparse

import numpy as np
import pytest
import torch

from serverless_learn_amd.data import augment as A


# ---- the permutation ----
@pytest.mark.parametrize("n", [1, 2, 3, 5, 32, 33, 37, 101, 4097, 127388])
def test_perm_is_a_bijection(n):
    for e in (0, 1, 2):
        out = A.perm(0, e, n, np.arange(n))
        assert out.dtype == np.int64 and np.array_equal(np.sort(out), np.arange(n)), (n, e)


def test_perm_shuffles():
    n = 101
    heads = {tuple(A.perm(0, e, n, np.arange(32))) for e in range(50)}
    assert len(heads) == 50 and tuple(range(32)) not in heads
    first = np.array([int(A.perm(0, e, n, np.array([0]))[0]) for e in range(2000)])
    counts = np.bincount(first, minlength=n)
    print("position-0 counts over 2000 epochs: min", counts.min(), "max", counts.max())
    assert counts.min() >= 1 and counts.max() <= 60  # expectation 19.8


def test_perm_is_vectorised_and_checked():
    n = 37
    q = np.array([[0, 5, 36], [7, 7, 1]])
    out = A.perm(3, 2, n, q)
    assert out.shape == q.shape
    for idx in np.ndindex(q.shape):
        assert out[idx] == A.perm(3, 2, n, np.array([q[idx]]))[0]
    with pytest.raises(ValueError):
        A.perm(0, 0, n, np.array([n]))
    assert not np.array_equal(A.perm(0, 0, n, np.arange(n)), A.perm(1 << 32, 0, n, np.arange(n)))  # k1 is used


# ---- the draws ----
@pytest.mark.parametrize("seed", [0, 7])
def test_draws_cover_their_range(seed):
    pad = 4
    oy, ox, flip = (np.concatenate(v) for v in zip(*[A.draws(seed, t, 1024, pad) for t in range(10)]))
    assert oy.min() == 0 and oy.max() == 2 * pad and ox.min() == 0 and ox.max() == 2 * pad
    pairs = np.bincount(oy * (2 * pad + 1) + ox, minlength=81)
    print("seed", seed, "min pair count", pairs.min(), "flip share", flip.mean())
    assert len(pairs) == 81 and pairs.min() >= 64  # half the expectation of 126.4
    assert 0.48 <= flip.mean() <= 0.52
    assert set(np.unique(flip)) == {0, 1}


# ---- off states and purity ----
def test_off_states_are_the_plain_batch():
    n, batch, pad = 37, 5, 3
    x = np.random.default_rng(0).integers(0, 256, size=(n, 6, 6, 3), dtype=np.uint8)
    for t in (0, 3, 7, 20):
        b = t % (n // batch)
        plain = np.arange(b * batch, (b + 1) * batch)
        off = A.batch_params(9, t, n, batch, pad, False, "none")
        assert off.dtype == np.int32 and off.shape == (batch, 4)
        assert np.array_equal(off, np.column_stack([plain, [pad] * batch, [pad] * batch, [0] * batch]))
        assert np.array_equal(A.apply(x, off, pad), x[plain])
        shuf = A.batch_params(9, t, n, batch, pad, True, "none")
        assert np.array_equal(shuf[:, 1:], off[:, 1:])
        assert np.array_equal(shuf[:, 0], A.perm(9, t // (n // batch), n, plain))
        assert np.array_equal(A.apply(x, shuf, pad), x[shuf[:, 0]])
        aug = A.batch_params(9, t, n, batch, pad, False, "crop-flip")
        assert np.array_equal(aug[:, 0], plain)
        oy, ox, flip = A.draws(9, t, batch, pad)
        assert np.array_equal(aug[:, 1:], np.column_stack([oy, ox, flip]))


def test_batch_params_is_pure():
    args = (5, 11, 101, 32, 4, True, "crop-flip")
    a, b = A.batch_params(*args), A.batch_params(*args)
    assert np.array_equal(a, b)
    # vectorised == per element: every sample's row on its own
    e, bb = divmod(11, 101 // 32)
    for j in range(32):
        oy, ox, flip = A.draws(5, 11, j + 1, 4)
        row = (int(A.perm(5, e, 101, np.array([bb * 32 + j]))[0]), oy[j], ox[j], flip[j])
        assert tuple(a[j]) == row
    assert not np.array_equal(a, A.batch_params(5, 12, 101, 32, 4, True, "crop-flip"))
    assert not np.array_equal(a, A.batch_params(6, 11, 101, 32, 4, True, "crop-flip"))
    with pytest.raises(ValueError):
        A.batch_params(0, 0, 101, 32, 4, False, "mixup")
    with pytest.raises(ValueError):
        A.batch_params(0, 0, 3, 4, 1, False, "none")


# ---- padding against a hand-written loop ----
@pytest.mark.parametrize("oy,ox", [(0, 0), (4, 4), (2, 2), (1, 3)])
@pytest.mark.parametrize("flip", [0, 1])
def test_apply_matches_a_loop(oy, ox, flip):
    hw, pad = 5, 2
    x = np.arange(1, 2 * hw * hw * 3 + 1, dtype=np.uint8).reshape(2, hw, hw, 3)  # no zero pixel in the image
    params = np.array([[1, oy, ox, flip]], np.int32)
    want = np.zeros((1, hw, hw, 3), np.uint8)
    for y in range(hw):
        for xx in range(hw):
            sy, sx = y + oy - pad, (hw - 1 - xx if flip else xx) + ox - pad
            if 0 <= sy < hw and 0 <= sx < hw:
                want[0, y, xx] = x[1, sy, sx]
    got = A.apply(x, params, pad)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    inside = sum(0 <= y + oy - pad < hw for y in range(hw)) * sum(0 <= c + ox - pad < hw for c in range(hw))
    assert int((got != 0).all(axis=-1).sum()) == inside  # the padded area is u8 0, the rest is image
    if (oy, ox, flip) == (pad, pad, 0):
        assert np.array_equal(got[0], x[1])


# ---- the CPU trainer ----
def _tiny_shard(n=9, hw=8):
    rng = np.random.default_rng(1)
    return (torch.from_numpy(rng.integers(0, 256, size=(n, hw, hw, 3), dtype=np.uint8)),
            torch.from_numpy(rng.integers(0, 10, size=n, dtype=np.uint8)))


def test_cpu_trainer_draws_the_reference_batches():
    from serverless_learn_amd.models.resnet import CPUResNetTrainer

    x, y = _tiny_shard()
    tr = CPUResNetTrainer(batch=4, in_hw=8, seed=3, augment="crop-flip", shuffle=True)
    tr.load_shard(x, y)
    assert tr.last_aug is None
    for t in range(3):
        assert tr.cursor == t
        tr.step()
        assert np.array_equal(tr.last_aug, A.batch_params(3, t, 9, 4, 4, True, "crop-flip"))
        assert np.isfinite(tr.stats().loss)
    plain = CPUResNetTrainer(batch=4, in_hw=8, seed=3)
    plain.load_shard(x, y)
    plain.step()
    assert plain.last_aug is None and (plain.augment, plain.augment_pad, plain.shuffle) == ("none", 4, False)


def test_trainers_refuse_bad_settings():
    from serverless_learn_amd.models.resnet import CPUResNetTrainer

    with pytest.raises(ValueError, match="augment"):
        CPUResNetTrainer(batch=4, in_hw=8, augment="mixup")
    with pytest.raises(ValueError, match="augment_pad"):
        CPUResNetTrainer(batch=4, in_hw=8, augment="crop-flip", augment_pad=-1)
    with pytest.raises(ValueError, match="augment_pad"):
        CPUResNetTrainer(batch=4, in_hw=8, augment="crop-flip", augment_pad=8)
    CPUResNetTrainer(batch=4, in_hw=8, augment="crop-flip", augment_pad=7)


# ---- configuration and worker ----
def test_config_env_and_cli_spellings(monkeypatch):
    from serverless_learn_amd import config as C

    d = C.Config()
    assert (d.augment, d.augment_pad, d.shuffle) == ("none", 4, False)
    for k, v in (("SL_MODEL", "resnet18"), ("SL_AUGMENT", "crop-flip"), ("SL_AUGMENT_PAD", "2"), ("SL_SHUFFLE", "1")):
        monkeypatch.setenv(k, v)
    e = C.Config.from_env()
    assert (e.model, e.augment, e.augment_pad, e.shuffle) == ("resnet18", "crop-flip", 2, True)
    for k in ("SL_MODEL", "SL_AUGMENT", "SL_AUGMENT_PAD", "SL_SHUFFLE"):
        monkeypatch.delenv(k)
    ap = argparse.ArgumentParser()
    C.add_cli_args(ap)
    a = C.from_args(ap.parse_args(["--model", "resnet18", "--augment", "crop-flip", "--augment-pad", "3",
                                   "--shuffle", "true"]))
    assert (a.model, a.augment, a.augment_pad, a.shuffle) == ("resnet18", "crop-flip", 3, True)
    n = C.from_args(ap.parse_args([]))
    assert (n.augment, n.augment_pad, n.shuffle) == ("none", 4, False)


@pytest.mark.parametrize("model", ["mlp", "simulate"])
@pytest.mark.parametrize("kw", [dict(augment="crop-flip"), dict(shuffle=True)])
def test_config_refuses_the_pipeline_without_a_resnet(model, kw):
    from serverless_learn_amd.config import Config

    with pytest.raises(ValueError, match="input pipeline"):
        Config(model=model, **kw)
    Config(model="resnet18", **kw)


def _worker(**kw):
    from serverless_learn_amd.runtime.local_cluster import fast_config
    from serverless_learn_amd.runtime.worker import Worker

    return Worker("127.0.0.1:0", fast_config(batch=4, model="resnet18", **kw))


def test_worker_passes_the_settings_only_when_set(monkeypatch):
    from serverless_learn_amd.runtime import worker as W

    seen = []
    real = W.make_trainer

    def spy(model, device, **kw):
        seen.append(kw)
        return real(model, device, **kw)

    monkeypatch.setattr(W, "make_trainer", spy)
    w = _worker(augment="crop-flip", augment_pad=2, shuffle=True)
    w._ensure_trainer()
    tr = w.trainer
    assert (tr.augment, tr.augment_pad, tr.shuffle, tr.seed) == ("crop-flip", 2, True, w.cfg.seed)
    assert {k: seen[-1][k] for k in ("augment", "augment_pad", "shuffle")} == dict(
        augment="crop-flip", augment_pad=2, shuffle=True)
    s = _worker(shuffle=True)
    s._ensure_trainer()
    assert (s.trainer.augment, s.trainer.augment_pad, s.trainer.shuffle) == ("none", 4, True)
    d = _worker()
    d._ensure_trainer()
    assert (d.trainer.augment, d.trainer.augment_pad, d.trainer.shuffle) == ("none", 4, False)
    assert not {"augment", "augment_pad", "shuffle"} & set(seen[-1])
    with pytest.raises(ValueError, match="augment"):
        _worker(augment="mixup")._ensure_trainer()
    with pytest.raises(ValueError, match="augment_pad"):
        _worker(augment="crop-flip", augment_pad=32)._ensure_trainer()
