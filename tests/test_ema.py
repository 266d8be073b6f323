"""The weight EMA on the CPU: the coefficient table, the three-rounding update (ops/optim.py
ema_update_, the reference the GPU kernel is held to in test_ema_gpu.py), both CPU trainers (the
definition on the trainers), the checkpoint round trip, the configuration and a worker.

After every optimizer update, ``e <- e + omd_t * (w - e)`` in fp32 (subtract, multiply, add, each rounded
once) with ``omd_t = float32(1 - d_t)`` and ``d_t = min(D, (1 + t) / (10 + t))`` under warm-up; ``t`` counts
EMA updates.  Everything here is an equality of bits.
"""
import argparse

import numpy as np
import pytest
import torch

from serverless_learn_amd.ckpt import format as ckfmt
from serverless_learn_amd.config import Config, add_cli_args, from_args
from serverless_learn_amd.data.synthetic import make_cifar_like, make_mnist_like
from serverless_learn_amd.models import make_trainer
from serverless_learn_amd.models import mlp as M
from serverless_learn_amd.models import resnet as R
from serverless_learn_amd.ops import optim as O

D, STEPS = 0.5, 12


# ---- the table ----
def test_table_values_and_lengths():
    tab = O.ema_table(0.5, True)
    assert tab.dtype == np.float32 and tab.shape == (9,)
    want = [np.float32(1.0 - min(0.5, (1 + t) / (10 + t))) for t in range(9)]
    assert [x.tobytes() for x in tab] == [x.tobytes() for x in want]
    assert tab[-1] == np.float32(0.5) and tab[0] == np.float32(0.9) and (np.diff(tab) < 0).all()
    assert (1 + 7) / (10 + 7) < 0.5 <= (1 + 8) / (10 + 8)  # T = 8 is the first t at the plateau
    off = O.ema_table(0.999, False)
    assert off.shape == (1,) and off[0] == np.float32(1.0 - 0.999)
    long = O.ema_table(0.9999, True)
    assert long.shape == (89_991,) and long[-1] == np.float32(1.0 - 0.9999) and long[-2] > long[-1]
    assert O.ema_table(0.05, True).shape == (1,)  # (1 + 0) / (10 + 0) >= D already
    assert O.ema_table_len(0.5) == 9 and O.ema_table_len(0.0) == 0
    assert O.OptSpec(ema_decay=0.5).ema_table().shape == (9,) and O.OptSpec().ema_table() is None


def test_table_refusals():
    for bad in (-0.1, float("nan"), 1.0, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            O.ema_table(bad, True)
        with pytest.raises(ValueError, match="ema_decay"):
            O.OptSpec(ema_decay=bad)
    d = 1.0 - 1e-7  # T ~ 9e7 > 2^20
    with pytest.raises(ValueError, match="ema_warmup off"):
        O.ema_table(d, True)
    with pytest.raises(ValueError, match="ema_warmup off"):
        O.OptSpec(ema_decay=d)
    assert O.ema_table(d, False).shape == (1,) and O.OptSpec(ema_decay=d, ema_warmup=False).emas
    with pytest.raises(ValueError):
        O.ema_table(0.0, True)  # off: no table


def test_optspec_rule_does_not_depend_on_the_ema():
    for kw in (dict(), dict(optimizer="adamw"), dict(lr_warmup_steps=3)):
        a, b = O.OptSpec(**kw), O.OptSpec(ema_decay=0.9, ema_warmup=False, **kw)
        assert (a.plain, a.rule, a.adamw, a.scheduled, a.clips) == (b.plain, b.rule, b.adamw, b.scheduled, b.clips)
        assert not a.emas and b.emas
        assert "ema_decay" not in a.meta() and (b.meta()["ema_decay"], b.meta()["ema_warmup"]) == (0.9, False)


# ---- the update ----
def test_update_is_three_roundings_and_w_equal_e_is_a_fixed_point():
    g = torch.Generator().manual_seed(0)
    e0, w = torch.randn(4099, generator=g), torch.randn(4099, generator=g)
    e0[::100] *= 1e3
    for omd in (np.float32(0.9), np.float32(1.0 - 0.9999), np.float32(0.5294118)):
        e = e0.clone()
        O.ema_update_(e, w, omd)
        d = (w.double() - e0.double()).float()            # rounded once
        p = (float(omd) * d.double()).float()             # rounded once (a 24 x 24-bit product is exact in fp64)
        want = (e0.double() + p.double()).float()         # rounded once
        assert torch.equal(e, want)
        assert torch.equal(e, e0 + torch.tensor(omd) * (w - e0))  # torch's fp32 expression
        fused = (e0.double() + float(omd) * (w.double() - e0.double())).float()
        assert not torch.equal(e, fused)  # (one rounding would differ: the three are observable)
        same = w.clone()
        O.ema_update_(same, w, omd)
        assert torch.equal(same, w)


# ---- the CPU trainers ----
def _mnist(batches, batch, seed=2):
    x, y = make_mnist_like(batches * batch, seed=seed)
    return torch.from_numpy(x), torch.from_numpy(y)


def _cifar(batches, batch, seed=3):
    x, y = make_cifar_like(batches * batch, seed=seed)
    return torch.from_numpy(x), torch.from_numpy(y)


def _mlp(seed=1, **kw):
    tr = M.CPUTrainer(batch=32, seed=seed, lr=0.1, momentum=0.9, **kw)
    tr.load_shard(*_mnist(4, 32))
    return tr


def _resnet(seed=5, **kw):
    tr = R.CPUResNetTrainer(batch=4, seed=seed, optimizer="adamw", lr=1e-3, **kw)
    tr.load_shard(*_cifar(3, 4))
    return tr


def _recurrence(e, w, t, tab):
    return e + tab[min(t, tab.numel() - 1)] * (w - e)


@pytest.mark.parametrize("make,steps", [(_mlp, STEPS), (_resnet, STEPS)], ids=["mlp", "resnet18"])
def test_cpu_trainer_follows_the_recurrence_and_trains_as_before(make, steps):
    tr, plain = make(ema_decay=D), make()
    tab = torch.from_numpy(O.ema_table(D, True))
    assert tr.ema_tab.numel() == 9 and torch.equal(tr.ema_tab, tab)
    assert plain.ema is None and plain.ema_step is None and plain.ema_tab is None
    e = tr.get_flat()
    assert torch.equal(tr.ema_flat(), e) and int(tr.ema_step[0]) == 0  # starts at the initial parameters
    for t in range(steps):  # passes the saturation at t = 8
        tr.step()
        plain.step()
        w = tr.get_flat()
        assert torch.equal(w, plain.get_flat()), t  # training is unaffected
        e = _recurrence(e, w, t, tab)
        assert torch.equal(tr.ema_flat(), e), t
        assert int(tr.ema_step[0]) == t + 1
    assert not torch.equal(tr.ema_flat(), tr.get_flat())
    if tr.mom is not None:
        assert torch.equal(tr.mom, plain.mom)
    tr.ema_flat().zero_()  # a clone
    assert torch.equal(tr.ema_flat(), e)


def test_starts_from_flat_and_one_update_per_accumulated_step():
    flat = M.init_params(9)
    tr = M.CPUTrainer(batch=32, flat=flat, ema_decay=D, accum_steps=2)
    tr.load_shard(*_mnist(4, 32))
    assert torch.equal(tr.ema_flat(), flat)
    tab, e = tr.ema_tab, flat.clone()
    for t in range(3):
        tr.step()
        e = _recurrence(e, tr.get_flat(), t, tab)
    assert int(tr.ema_step[0]) == 3 and tr.cursor == 6 and torch.equal(tr.ema_flat(), e)
    r = R.CPUResNetTrainer(batch=4, seed=5, ema_decay=D, ema_warmup=False, accum_steps=2)
    r.load_shard(*_cifar(2, 4))
    e = r.get_flat()
    r.step()
    assert r.ema_tab.numel() == 1 and int(r.ema_step[0]) == 1 and r.cursor == 2
    assert torch.equal(r.ema_flat(), e + r.ema_tab[0] * (r.get_flat() - e))


def test_set_flat_and_reset_leave_the_ema_alone():
    tr = _mlp(ema_decay=D)
    for _ in range(2):
        tr.step()
    e = tr.ema_flat()
    tr.set_flat(M.init_params(4))
    tr.refresh_shadows()
    tr.reset_optimizer_state()
    assert torch.equal(tr.ema_flat(), e) and int(tr.ema_step[0]) == 2


def test_evaluate_with_the_ema():
    x, y = _mnist(4, 32)
    tr = _mlp(ema_decay=D)
    for _ in range(3):
        tr.step()
    before = (tr.get_flat(), tr.ema_flat(), tr.mom.clone(), tr.cursor)
    got, own = tr.evaluate(x, y, ema=True), tr.evaluate(x, y)
    second = M.CPUTrainer(batch=32, seed=8)
    second.set_flat(tr.ema_flat())
    assert got == second.evaluate(x, y) and got != own and got.n == 128
    assert torch.equal(tr.get_flat(), before[0]) and torch.equal(tr.ema_flat(), before[1])
    assert torch.equal(tr.mom, before[2]) and tr.cursor == before[3]
    with pytest.raises(ValueError, match="ema"):
        _mlp().evaluate(x, y, ema=True)
    with pytest.raises(ValueError, match="ema"):
        _mlp().ema_flat()
    xc, yc = _cifar(3, 4)
    r = _resnet(ema_decay=D)
    for _ in range(2):
        r.step()
    stats = {k: (a.clone(), b.clone()) for k, (a, b) in r.running.items()}
    got = r.evaluate(xc, yc, ema=True)
    second = R.CPUResNetTrainer(batch=4, seed=9)
    second.set_flat(r.ema_flat())
    for k, (a, b) in r.running.items():  # the same running statistics: those are not averaged
        second.running[k][0].copy_(a)
        second.running[k][1].copy_(b)
        assert torch.equal(a, stats[k][0]) and torch.equal(b, stats[k][1])
    assert got == second.evaluate(xc, yc) and got != r.evaluate(xc, yc)
    with pytest.raises(ValueError, match="ema"):
        _resnet().evaluate(xc, yc, ema=True)


# ---- checkpoints ----
def _through_the_file(tr, step):
    n = tr.n_params
    buf = ckfmt.encode(tr.get_flat().numpy(), {"model": tr.model_name, "step": step}, tr.mom[:n].numpy(),
                       tr.state_extra())
    return ckfmt.decode_full(buf)


def _restore(tr, params, mom, extra):
    tr.set_flat(torch.from_numpy(params))  # the worker's order: the weights first
    tr.mom[:tr.n_params].copy_(torch.from_numpy(mom))
    tr.load_state_extra(extra)


@pytest.mark.parametrize("make", [_mlp, _resnet], ids=["mlp", "resnet18"])
def test_round_trip_through_the_checkpoint_format(make):
    a = make(ema_decay=D)
    for _ in range(5):
        a.step()
    meta, params, mom, extra = _through_the_file(a, 5)
    assert int(extra["ema_step"][0]) == 5 and extra["ema"].size == a.n_params
    assert torch.equal(torch.from_numpy(extra["ema"]).float(), a.ema_flat())
    b = make(seed=77, ema_decay=D)  # another init: everything must come from the file
    assert not torch.equal(b.ema_flat(), a.ema_flat())
    _restore(b, params, mom, extra)
    for _ in range(5):
        a.step()
        b.step()
    assert torch.equal(a.ema_flat(), b.ema_flat()) and torch.equal(a.get_flat(), b.get_flat())
    assert int(a.ema_step[0]) == int(b.ema_step[0]) == 10
    straight = make(ema_decay=D)
    for _ in range(10):
        straight.step()
    assert torch.equal(straight.ema_flat(), b.ema_flat()) and int(straight.ema_step[0]) == 10


def test_checkpoints_without_the_keys_and_trainers_without_the_ema():
    plain = _mlp()
    for _ in range(3):
        plain.step()
    meta, params, mom, extra = _through_the_file(plain, 3)
    assert sorted(extra) == ["cursor"]  # exactly what it was
    b = _mlp(seed=77, ema_decay=D)
    b.step()
    _restore(b, params, mom, extra)
    assert torch.equal(b.ema_flat(), plain.get_flat()) and int(b.ema_step[0]) == 0  # from the loaded weights
    half = dict(extra, ema=np.zeros(b.n_params))  # one key of the two: as if absent
    b.step()
    b.load_state_extra(half)
    assert torch.equal(b.ema_flat(), b.get_flat()) and int(b.ema_step[0]) == 0
    # an EMA checkpoint into a trainer without one: the keys are ignored
    a = _mlp(ema_decay=D)
    for _ in range(3):
        a.step()
    meta, params, mom, extra = _through_the_file(a, 3)
    assert sorted(extra) == ["cursor", "ema", "ema_step"]
    c = _mlp(seed=77)
    _restore(c, params, mom, extra)
    assert c.ema is None and torch.equal(c.get_flat(), a.get_flat()) and c.cursor == 3
    c.step()
    a.step()
    assert torch.equal(c.get_flat(), a.get_flat())


def test_buffers_and_state_keys_only_when_on():
    for make, base in ((_mlp, ["cursor"]), (_resnet, None)):
        off, on = make(), make(ema_decay=D)
        keys_off, keys_on = sorted(off.state_extra()), sorted(on.state_extra())
        assert "ema" not in keys_off and "ema_step" not in keys_off
        assert sorted(keys_off + ["ema", "ema_step"]) == keys_on
        if base is not None:
            assert keys_off == base
        assert len(on.buffers()) == len(off.buffers()) + 2
        assert on.buffers()[-2] is on.ema and on.buffers()[-1] is on.ema_step
        assert all(t is not off.params for t in off.buffers())
    adam = _resnet()
    assert sorted(k for k in adam.state_extra() if not k.startswith("bn/")) == ["cursor", "exp_avg_sq", "opt_step"]


# ---- configuration ----
def test_config_refusals_and_spelling(monkeypatch):
    assert (Config().ema_decay, Config().ema_warmup) == (0.0, True)
    Config(ema_decay=0.999, model="resnet18")
    Config(ema_decay=1.0 - 1e-7, ema_warmup=False)
    for bad in (dict(ema_decay=-0.5), dict(ema_decay=float("nan")), dict(ema_decay=1.0), dict(ema_decay=2.0),
                dict(ema_decay=0.5, model="simulate"), dict(ema_decay=1.0 - 1e-7)):
        with pytest.raises(ValueError):
            Config(**bad)
    with pytest.raises(ValueError, match="ema_warmup off"):
        Config(ema_decay=1.0 - 1e-7)
    cfg = Config()
    cfg.ema_decay = 1.0  # set after construction: the worker validates again
    with pytest.raises(ValueError):
        cfg.validate()
    ap = argparse.ArgumentParser()
    add_cli_args(ap)
    cfg = from_args(ap.parse_args(["--ema-decay", "0.99", "--ema-warmup", "false"]))
    assert (cfg.ema_decay, cfg.ema_warmup) == (0.99, False)
    monkeypatch.setenv("SL_EMA_DECAY", "0.9")
    monkeypatch.setenv("SL_EMA_WARMUP", "0")
    cfg = Config.from_env()
    assert (cfg.ema_decay, cfg.ema_warmup) == (0.9, False)
    assert from_args(ap.parse_args(["--ema-decay", "0.5"])).ema_decay == 0.5  # the flag wins
    monkeypatch.setenv("SL_EMA_DECAY", "1")
    with pytest.raises(ValueError):
        Config.from_env()


def test_make_trainer_passes_the_settings():
    for model, batch in (("mlp", 8), ("resnet18", 4)):
        tr = make_trainer(model, torch.device("cpu"), batch=batch, ema_decay=0.9, ema_warmup=False)
        assert tr.opt.ema_decay == 0.9 and tr.ema_tab.numel() == 1 and tr.ema.shape == tr.params.shape
        assert make_trainer(model, torch.device("cpu"), batch=batch).ema is None


# ---- the worker ----
def test_worker_trains_logs_checkpoints_and_a_second_one_resumes(monkeypatch):
    from serverless_learn_amd.runtime.local_cluster import LocalCluster, fast_config
    from serverless_learn_amd.utils.log import Logger

    events = []
    emit = Logger._emit
    monkeypatch.setattr(Logger, "_emit", lambda self, level, event, **f: (events.append((self.addr, event, f)),
                                                                           emit(self, level, event, **f))[1])
    B, steps = 64, 20
    c = LocalCluster(fast_config(batch=B, shard_records=8 * B, log_every=10, ema_decay=D, max_steps=steps))
    try:
        a = c.add_worker(sync="none")
        assert c.wait_for(lambda: a.state == "done", 60), (a.state, a.step)
        t = a.trainer
        assert a.step == steps and int(t.ema_step[0]) == steps
        assert [f for addr, e, f in events if e == "ema"] == [{"decay": D, "warmup": True, "table": 9}]
        # the bare trainer on the same shard
        eng = M.CPUTrainer(batch=B, lr=a.cfg.lr, momentum=a.cfg.momentum, weight_decay=a.cfg.weight_decay,
                           seed=a.cfg.seed, ema_decay=D)
        eng.load_shard(t.x, t.y)
        for _ in range(steps):
            eng.step()
        assert torch.equal(eng.get_flat(), t.get_flat()) and torch.equal(eng.ema_flat(), t.ema_flat())
        fn = a.save_checkpoint()
        meta, params, mom, extra = ckfmt.decode_full(c.file_server.get_file(fn))
        assert meta["optimizer"]["ema_decay"] == D and meta["optimizer"]["ema_warmup"] is True
        assert {"ema", "ema_step"} <= set(extra) and int(extra["ema_step"][0]) == steps
        # a second worker, another seed: it resumes from the checkpoint with an identical EMA and takes it on;
        # the bare trainer restored from the same file and stepped on the same shard is the reference
        more = 4
        b = c.add_worker(sync="none", seed=5, max_steps=steps + more)
        assert c.wait_for(lambda: b.resumed_step == steps and b.state == "done", 60), (b.state, b.step, b.resumed_step)
        assert b.step == steps + more and int(b.trainer.ema_step[0]) == steps + more
        ref = M.CPUTrainer(batch=B, lr=a.cfg.lr, momentum=a.cfg.momentum, weight_decay=a.cfg.weight_decay, seed=99,
                           ema_decay=D)
        _restore(ref, params, mom, extra)
        assert torch.equal(ref.ema_flat(), t.ema_flat()) and int(ref.ema_step[0]) == steps
        ref.load_shard(b.trainer.x, b.trainer.y)
        for _ in range(more):
            ref.step()
        assert torch.equal(b.trainer.ema_flat(), ref.ema_flat()) and torch.equal(b.trainer.get_flat(), ref.get_flat())
        assert not [e for addr, e, f in events if e == "checkpoint_ema_missing"]
        # a checkpoint without the keys into an EMA trainer: from the loaded weights, and said so
        old = ckfmt.encode(params, dict({k: v for k, v in meta.items() if k != "extra"}, step=b.step), mom,
                           {k: v for k, v in extra.items() if k not in ("ema", "ema_step")})
        b._load_checkpoint(old)
        assert [addr for addr, e, f in events if e == "checkpoint_ema_missing"] == [b.addr]
        assert torch.equal(b.trainer.ema_flat(), b.trainer.get_flat()) and int(b.trainer.ema_step[0]) == 0
    finally:
        c.stop()
