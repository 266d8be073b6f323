"""Label smoothing, mixup and CutMix as defined in serverless_learn_amd/data/augment.py: the Beta
quantile table is symmetric, monotone and has the distribution's moments; the per-batch draw pairs
every sample with another one and reports the weight of what it pasted; the blend and the soft
targets are exact on hand-made cases; Config, the CLI and the CPU trainer carry the settings."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from serverless_learn_amd.data import augment as A

ALPHAS = (0.2, 0.4, 1, 2, 8)
L = A.MIX_L


def _kc(alpha):
    tab = A.mix_table(alpha)
    assert tab.dtype == np.int32 and tab.shape == (L,)
    return (tab & 0xFFFF).astype(np.int64), (tab >> 16).astype(np.int64)


# ---- the table ----
@pytest.mark.parametrize("alpha", ALPHAS)
def test_table_is_symmetric_monotone_and_has_the_moments(alpha):
    k, c = _kc(alpha)
    assert (np.diff(k) >= 0).all() and k.min() >= 0 and k.max() <= 256
    assert (k + k[::-1] == 256).all()
    assert int(k.sum()) * 2 == 256 * L  # mean lambda is exactly 1/2
    var, want = (k / 256.0).var(), 1.0 / (4 * (2 * alpha + 1))
    print(f"alpha {alpha}: var {var:.9f} want {want:.9f} rel {var / want - 1:+.2e}")
    assert abs(var / want - 1) <= 1e-3
    assert c.min() >= 0 and c.max() <= 256 and (np.diff(c) <= 0).all()
    q = A.beta_quantiles(alpha, L)
    assert q.dtype == np.float64 and q.shape == (L,) and (np.diff(q) >= 0).all() and 0 <= q[0] and q[-1] <= 1
    assert np.array_equal(k, np.floor(256 * q + 0.5)) and np.array_equal(c, np.floor(256 * np.sqrt(1 - q) + 0.5))


def test_uniform_quantiles_are_the_midpoints():
    assert np.abs(A.beta_quantiles(1.0, L) - (np.arange(L) + 0.5) / L).max() < 1e-14


@pytest.mark.parametrize("alpha", ALPHAS)
def test_quantiles_against_scipy(alpha):
    sp = pytest.importorskip("scipy.special")
    err = np.abs(A.beta_quantiles(alpha, L) - sp.betaincinv(alpha, alpha, (np.arange(L) + 0.5) / L)).max()
    print(f"alpha {alpha}: max |Q - betaincinv| = {err:.2e}")
    assert err <= 1e-9


def test_mix_tables_rows_and_the_off_row():
    t = A.mix_tables(0.4, 2.0)
    assert t.dtype == np.int32 and t.shape == (2, L)
    assert np.array_equal(t[0], A.mix_table(0.4)) and np.array_equal(t[1], A.mix_table(2.0))
    off = A.mix_tables(0.0, 1.0)[0]
    assert (off == 256).all()  # k = 256, c = 0: no mixing


# ---- the per-batch draw ----
@pytest.mark.parametrize("batch", [2, 3, 4, 32])
def test_partner_is_a_rotation_without_fixed_point(batch):
    rs = set()
    for t in list(range(40)) + [2**31 - 1, 2_000_000_011]:
        m = A.mix_params(7, t, batch, 8, 8, 1.0, 1.0)
        assert m.dtype == np.int32 and m.shape == (batch, 8)
        pj = m[:, 0]
        assert sorted(pj.tolist()) == list(range(batch)) and (pj != np.arange(batch)).all(), t
        rs.add(int((pj[0] - 0) % batch))
        assert (m[:, 1:] == m[0, 1:]).all()  # one draw per batch
    assert rs <= set(range(1, batch)) and (batch > 4 or rs == set(range(1, batch))) and (batch == 2 or len(rs) > 1)


@pytest.mark.parametrize("hw", [(8, 8), (5, 9), (32, 32)])
def test_weights_and_box(hw):
    H, W = hw
    modes, areas = set(), set()
    for t in range(200):
        m = A.mix_params(3, t, 4, H, W, 0.4, 1.0)[0]
        _, num, den, mode, x0, y0, x1, y1 = (int(v) for v in m)
        modes.add(mode)
        assert 0 <= num <= den
        if mode == A.MODE_MIXUP:
            assert den == 256 and (x0, y0, x1, y1) == (0, 0, 0, 0)
        else:
            assert mode == A.MODE_CUTMIX and den == H * W
            assert 0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H and num == (x1 - x0) * (y1 - y0)
            areas.add(num)
    assert modes == {A.MODE_MIXUP, A.MODE_CUTMIX} and len(areas) > 3
    assert {int(A.mix_params(3, t, 4, H, W, 0.4, 0.0)[0, 3]) for t in range(20)} == {A.MODE_MIXUP}
    assert {int(A.mix_params(3, t, 4, H, W, 0.0, 1.0)[0, 3]) for t in range(20)} == {A.MODE_CUTMIX}


def test_box_follows_the_definition():
    """The draw re-derived by hand from the two Philox words."""
    from serverless_learn_amd.data.device_synth import philox4x32_10

    H, W, seed = 6, 10, 11 + (5 << 32)
    tab = A.mix_table(1.0)
    for t in (0, 1, 17, 2**31 - 1):
        m = [int(v) for v in philox4x32_10(t, 0, 0, 3, seed & 0xFFFFFFFF, seed >> 32)]
        n = [int(v) for v in philox4x32_10(t, 1, 0, 3, seed & 0xFFFFFFFF, seed >> 32)]
        c = (int(tab[m[0] >> 20]) >> 16) & 0xFFFF
        bw, bh = (W * c + 128) >> 8, (H * c + 128) >> 8
        cx, cy = n[0] % W, n[1] % H
        box = (max(cx - bw // 2, 0), max(cy - bh // 2, 0), min(cx - bw // 2 + bw, W), min(cy - bh // 2 + bh, H))
        if bw == 0 or bh == 0:
            box = (0, 0, 0, 0)
        got = A.mix_params(seed, t, 3, H, W, 0.0, 1.0)
        assert tuple(int(v) for v in got[0, 4:]) == box
        assert np.array_equal(got[:, 0], (np.arange(3) + 1 + m[1] % 2) % 3)


def test_seeds_differ():
    a = np.stack([A.mix_params(5, t, 32, 32, 32, 1.0, 1.0) for t in range(8)])
    assert np.array_equal(a, np.stack([A.mix_params(5, t, 32, 32, 32, 1.0, 1.0) for t in range(8)]))
    assert not np.array_equal(a, np.stack([A.mix_params(6, t, 32, 32, 32, 1.0, 1.0) for t in range(8)]))
    assert not np.array_equal(a, np.stack([A.mix_params(5 + (1 << 32), t, 32, 32, 32, 1.0, 1.0) for t in range(8)]))


def test_mix_params_refuses_bad_arguments():
    with pytest.raises(ValueError, match="batch"):
        A.mix_params(0, 0, 1, 8, 8, 1.0, 0.0)
    with pytest.raises(ValueError):
        A.mix_params(0, 0, 4, 8, 8, 0.0, 0.0)
    with pytest.raises(ValueError, match="mixup_alpha"):
        A.mix_params(0, 0, 4, 8, 8, -1.0, 0.0)


# ---- the blend and the targets ----
def _two():
    return np.arange(2 * 4 * 4 * 3, dtype=np.uint8).reshape(2, 4, 4, 3) * 2 + 1


def test_mix_apply_mixup_by_hand():
    x = _two()
    mix = np.array([[1, 256 - 64, 256, 1, 0, 0, 0, 0], [0, 256 - 64, 256, 1, 0, 0, 0, 0]], np.int32)  # k = 64
    got = A.mix_apply(x, mix)
    assert got.dtype == np.float32 and got.shape == x.shape
    want = (64 * x.astype(np.float64) + 192 * x[::-1].astype(np.float64)) / 256
    assert np.array_equal(got.astype(np.float64), want)  # exact: multiples of 1/256 below 256
    same = A.mix_apply(x, np.array([[1, 0, 256, 1, 0, 0, 0, 0], [0, 0, 256, 1, 0, 0, 0, 0]], np.int32))  # k = 256
    assert np.array_equal(same, x.astype(np.float32))
    swap = A.mix_apply(x, np.array([[1, 256, 256, 1, 0, 0, 0, 0], [0, 256, 256, 1, 0, 0, 0, 0]], np.int32))  # k = 0
    assert np.array_equal(swap, x[::-1].astype(np.float32))


def test_mix_apply_cutmix_by_hand():
    x = _two()
    mix = np.array([[1, 6, 16, 2, 1, 0, 4, 2], [0, 6, 16, 2, 1, 0, 4, 2]], np.int32)  # columns 1-3 of rows 0-1
    got = A.mix_apply(x, mix)
    want = x.copy()
    want[0, 0:2, 1:4], want[1, 0:2, 1:4] = x[1, 0:2, 1:4], x[0, 0:2, 1:4]
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    empty = A.mix_apply(x, np.array([[1, 0, 16, 2, 0, 0, 0, 0], [0, 0, 16, 2, 0, 0, 0, 0]], np.int32))
    assert np.array_equal(empty, x.astype(np.float32))
    full = A.mix_apply(x, np.array([[1, 16, 16, 2, 0, 0, 4, 4], [0, 16, 16, 2, 0, 0, 4, 4]], np.int32))
    assert np.array_equal(full, x[::-1].astype(np.float32))


def test_soft_targets():
    lab = np.array([3, 3, 9, 0], np.uint8)
    mix = np.array([[1, 64, 256, 1, 0, 0, 0, 0], [2, 64, 256, 1, 0, 0, 0, 0], [3, 64, 256, 1, 0, 0, 0, 0],
                    [0, 64, 256, 1, 0, 0, 0, 0]], np.int32)
    for eps in (0.0, 0.1):
        for m in (None, mix):
            q = A.soft_targets(lab, m, eps, 10)
            assert q.dtype == np.float64 and q.shape == (4, 10)
            assert np.abs(q.sum(1) - 1).max() < 1e-15 and (q >= 0).all()
    q = A.soft_targets(lab, mix, 0.1, 10)
    assert q[0, 3] == pytest.approx(0.9 + 0.01) and q[0, 0] == pytest.approx(0.01)  # partner has the same label
    assert q[1, 3] == pytest.approx(0.9 * 0.75 + 0.01) and q[1, 9] == pytest.approx(0.9 * 0.25 + 0.01)
    assert np.array_equal(A.soft_targets(lab, None, 0.0, 10), np.eye(10)[lab])
    t = torch.from_numpy(A.soft_targets(lab, None, 0.1, 10))
    z = torch.randn(4, 10, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    assert torch.allclose(F.cross_entropy(z, t), F.cross_entropy(z, torch.from_numpy(lab).long(), label_smoothing=0.1),
                          rtol=0, atol=1e-14)


# ---- settings ----
def test_config_env_and_cli_spellings(monkeypatch):
    from serverless_learn_amd import config as C

    d = C.Config()
    assert (d.label_smoothing, d.mixup_alpha, d.cutmix_alpha) == (0.0, 0.0, 0.0)
    env = (("SL_MODEL", "resnet18"), ("SL_LABEL_SMOOTHING", "0.1"), ("SL_MIXUP_ALPHA", "0.2"), ("SL_CUTMIX_ALPHA", "1"))
    for k, v in env:
        monkeypatch.setenv(k, v)
    e = C.Config.from_env()
    assert (e.model, e.label_smoothing, e.mixup_alpha, e.cutmix_alpha) == ("resnet18", 0.1, 0.2, 1.0)
    for k, _ in env:
        monkeypatch.delenv(k)
    ap = argparse.ArgumentParser()
    C.add_cli_args(ap)
    a = C.from_args(ap.parse_args(["--model", "resnet18", "--label-smoothing", "0.05", "--mixup-alpha", "0.4",
                                   "--cutmix-alpha", "1.0", "--augment", "crop-flip"]))
    assert (a.label_smoothing, a.mixup_alpha, a.cutmix_alpha, a.augment) == (0.05, 0.4, 1.0, "crop-flip")
    n = C.from_args(ap.parse_args([]))
    assert (n.label_smoothing, n.mixup_alpha, n.cutmix_alpha) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("model", ["mlp", "simulate"])
@pytest.mark.parametrize("kw", [dict(label_smoothing=0.1), dict(mixup_alpha=0.2), dict(cutmix_alpha=1.0)])
def test_config_refuses_the_settings_without_a_resnet(model, kw):
    from serverless_learn_amd.config import Config

    with pytest.raises(ValueError, match="resnet18"):
        Config(model=model, **kw)
    Config(model="resnet18", **kw)


@pytest.mark.parametrize("kw", [dict(label_smoothing=1.0), dict(label_smoothing=-0.1),
                                dict(label_smoothing=float("nan")), dict(mixup_alpha=-1.0),
                                dict(mixup_alpha=float("inf")), dict(mixup_alpha=float("nan")),
                                dict(cutmix_alpha=-0.5), dict(cutmix_alpha=float("inf")),
                                dict(cutmix_alpha=float("nan"))])
def test_bad_ranges_are_refused_everywhere(kw):
    from serverless_learn_amd.config import Config
    from serverless_learn_amd.models.resnet import CPUResNetTrainer

    with pytest.raises(ValueError, match=next(iter(kw))):
        Config(model="resnet18", **kw)
    with pytest.raises(ValueError, match=next(iter(kw))):
        CPUResNetTrainer(batch=4, in_hw=8, **kw)


def test_augment_is_not_the_spelling():
    from serverless_learn_amd.models.resnet import CPUResNetTrainer

    with pytest.raises(ValueError, match="augment"):
        CPUResNetTrainer(batch=4, in_hw=8, augment="mixup")
    with pytest.raises(ValueError, match="batch"):
        CPUResNetTrainer(batch=1, in_hw=8, mixup_alpha=0.2)
    with pytest.raises(ValueError, match="batch"):
        CPUResNetTrainer(batch=1, in_hw=8, cutmix_alpha=1.0)
    CPUResNetTrainer(batch=1, in_hw=8, label_smoothing=0.1)


def test_worker_passes_the_settings_only_when_set(monkeypatch):
    from serverless_learn_amd.runtime import worker as W
    from serverless_learn_amd.runtime.local_cluster import fast_config

    seen = []
    real = W.make_trainer

    def spy(model, device, **kw):
        seen.append(kw)
        return real(model, device, **kw)

    monkeypatch.setattr(W, "make_trainer", spy)
    keys = ("label_smoothing", "mixup_alpha", "cutmix_alpha")
    w = W.Worker("127.0.0.1:0", fast_config(batch=4, model="resnet18", label_smoothing=0.1, cutmix_alpha=1.0))
    w._ensure_trainer()
    assert {k: seen[-1][k] for k in keys} == dict(label_smoothing=0.1, mixup_alpha=0.0, cutmix_alpha=1.0)
    assert tuple(getattr(w.trainer, k) for k in keys) == (0.1, 0.0, 1.0) and w.trainer.augment == "none"
    d = W.Worker("127.0.0.1:0", fast_config(batch=4, model="resnet18"))
    d._ensure_trainer()
    assert not set(keys) & set(seen[-1]) and tuple(getattr(d.trainer, k) for k in keys) == (0.0, 0.0, 0.0)


# ---- the CPU trainer ----
def _tiny_shard(n=9, hw=8):
    rng = np.random.default_rng(1)
    return (torch.from_numpy(rng.integers(0, 256, size=(n, hw, hw, 3), dtype=np.uint8)),
            torch.from_numpy(rng.integers(0, 10, size=n, dtype=np.uint8)))


def _cpu(**kw):
    from serverless_learn_amd.models.resnet import CPUResNetTrainer

    tr = CPUResNetTrainer(batch=4, in_hw=8, seed=3, **kw)
    tr.load_shard(*_tiny_shard())
    return tr


def test_cpu_trainer_smoothing_is_torchs():
    from serverless_learn_amd.models.resnet import ref_forward

    tr = _cpu(label_smoothing=0.1)
    x, y = _tiny_shard()
    tr.step()
    flat = tr.params.clone()  # after one step; the second batch is records 4..7
    tr.step()
    assert tr.last_mix is None and tr.last_aug is None
    with torch.no_grad():
        logits = ref_forward(tr.spec, flat, x[4:8], True, None)
    want = F.cross_entropy(logits, y[4:8].long(), label_smoothing=0.1, reduction="sum")
    assert tr.stats().loss * 4 == pytest.approx(float(want), rel=1e-5)
    plain = F.cross_entropy(logits, y[4:8].long(), reduction="sum")
    assert abs(float(plain) - float(want)) > 1e-3  # the setting does something


def test_cpu_trainer_mixes_and_resumes():
    on = dict(mixup_alpha=0.4, cutmix_alpha=1.0, label_smoothing=0.1, augment="crop-flip", shuffle=True)
    a = _cpu(**on)
    assert a.last_mix is None
    seen = set()
    for t in range(3):
        a.step()
        assert np.array_equal(a.last_mix, A.mix_params(3, t, 4, 8, 8, 0.4, 1.0))
        assert np.array_equal(a.last_aug, A.batch_params(3, t, 9, 4, 4, True, "crop-flip"))
        seen.add(int(a.last_mix[0, 3]))
    extra = a.state_extra()
    assert "cursor" in extra and not any("mix" in k or "smooth" in k for k in extra)
    assert set(extra) == set(_cpu().state_extra())  # no new checkpoint key
    b = _cpu(**on)
    b.set_flat(a.get_flat())
    b.mom.copy_(a.mom)
    b.load_state_extra(extra)
    a.step()
    b.step()
    assert np.array_equal(a.last_aug, b.last_aug) and np.array_equal(a.last_mix, b.last_mix)
    assert np.array_equal(a.last_mix, A.mix_params(3, 3, 4, 8, 8, 0.4, 1.0))
    assert a.stats().loss == b.stats().loss and np.isfinite(a.stats().loss)
    assert torch.equal(a.get_flat(), b.get_flat())


def test_cpu_trainer_mix_alone_needs_no_pipeline():
    tr = _cpu(mixup_alpha=1.0)
    tr.step()
    tr.step()
    assert np.array_equal(tr.last_aug, A.batch_params(3, 1, 9, 4, 4, False, "none"))
    assert np.array_equal(tr.last_aug[:, 0], np.arange(4, 8)) and (tr.last_mix[:, 3] == A.MODE_MIXUP).all()
    assert np.isfinite(tr.stats().loss)
