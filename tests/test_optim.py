"""Optimizers and learning-rate schedules on the CPU: the reference semantics (ops/optim.py
``lr_at`` / ``adamw_update``) against their formulas and torch.optim, exact resume of the new
optimizer state, and the Config / worker / checkpoint wiring."""
import math

import pytest
import torch

from serverless_learn_amd.ckpt import format as ckfmt
from serverless_learn_amd.data.synthetic import make_mnist_like
from serverless_learn_amd.models import make_trainer
from serverless_learn_amd.models.mlp import MLP, CPUTrainer, init_params
from serverless_learn_amd.ops.optim import OptSpec, lr_at

ADAMW = dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2)


def _shard(n=256, seed=3):
    x, y = make_mnist_like(n, seed=seed)
    return torch.from_numpy(x), torch.from_numpy(y)


# ---- 1. lr_at ----
def test_lr_at_warmup_and_decay_shapes():
    lr, W, D, r = 0.2, 4, 20, 0.1
    for sched in ("constant", "linear", "cosine"):
        assert lr_at(0, lr, sched, W, D, r) == pytest.approx(lr / W, rel=1e-15)
        assert lr_at(W - 1, lr, sched, W, D, r) == pytest.approx(lr, rel=1e-15)
    # cosine: p = 1/2 at the midpoint of [W, D]
    assert lr_at(12, lr, "cosine", W, D, r) == pytest.approx(lr * (r + (1 - r) * 0.5), rel=1e-15)
    assert lr_at(8, lr, "cosine", W, D, r) == pytest.approx(lr * (r + (1 - r) * 0.5 * (1 + math.cos(math.pi / 4))),
                                                            rel=1e-15)
    assert lr_at(W, lr, "cosine", W, D, r) == pytest.approx(lr, rel=1e-15)
    assert lr_at(12, lr, "linear", W, D, r) == pytest.approx(lr * (r + (1 - r) * 0.5), rel=1e-15)
    for sched in ("linear", "cosine"):
        for step in (D, D + 1, 10 * D):
            assert lr_at(step, lr, sched, W, D, r) == pytest.approx(r * lr, rel=1e-12, abs=1e-18)
    # no warm-up: the first step runs at the full lr
    assert lr_at(0, lr, "cosine", 0, D, r) == pytest.approx(lr, rel=1e-15)


def test_lr_at_constant_ignores_decay_fields_and_decay_needs_a_horizon():
    for step in (0, 5, 10_000):
        assert lr_at(step, 0.3, "constant", 0, 7, 0.5) == 0.3
        assert lr_at(step, 0.3) == 0.3
    for sched in ("linear", "cosine"):
        with pytest.raises(ValueError, match="lr_decay_steps"):
            lr_at(3, 0.1, sched, 2, 0, 0.0)
        with pytest.raises(ValueError, match="lr_decay_steps"):
            OptSpec(lr_schedule=sched)
    with pytest.raises(ValueError, match="constant"):
        lr_at(0, 0.1, "step")


def test_lr_table_is_lr_at_and_flat_past_its_end():
    for spec in (OptSpec(lr=0.1, lr_schedule="cosine", lr_warmup_steps=3, lr_decay_steps=8, lr_min_ratio=0.05),
                 OptSpec(lr=0.1, lr_schedule="linear", lr_warmup_steps=5, lr_decay_steps=2),
                 OptSpec(lr=0.1, lr_warmup_steps=4)):
        tab = spec.lr_table()
        for s in range(len(tab) + 5):
            assert float(tab[min(s, len(tab) - 1)]) == pytest.approx(spec.lr_at(s), rel=1e-7, abs=1e-12), (spec, s)
    assert OptSpec().lr_table() is None and OptSpec(optimizer="adamw").lr_table() is None


# ---- 2. the CPU trainers against torch.optim ----
def _torch_run(opt_factory, sched_factory, x, y, batch, steps, seed):
    model = MLP(init_params(seed))
    opt = opt_factory([model.flat])
    sched = sched_factory(opt) if sched_factory else None
    nb = x.shape[0] // batch
    for s in range(steps):
        b = s % nb
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(x[b * batch:(b + 1) * batch]),
                                                 y[b * batch:(b + 1) * batch].long())
        loss.backward()
        opt.step()
        if sched:
            sched.step()
    return model.flat.detach()


def test_cpu_adamw_matches_torch():
    x, y = _shard()
    tr = CPUTrainer(batch=128, seed=1, **ADAMW)
    tr.load_shard(x, y)
    for _ in range(5):
        tr.step()
    ref = _torch_run(lambda p: torch.optim.AdamW(p, lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8),
                     None, x, y, 128, 5, 1)
    torch.testing.assert_close(tr.params, ref)
    assert int(tr.opt_step[0]) == 5 and tr.cursor == 5


def test_cpu_sgd_cosine_matches_torch_lambda_lr():
    x, y = _shard()
    lr, sch = 0.05, dict(lr_schedule="cosine", lr_warmup_steps=2, lr_decay_steps=5, lr_min_ratio=0.1)
    tr = CPUTrainer(batch=128, seed=1, lr=lr, momentum=0.9, weight_decay=1e-4, **sch)
    tr.load_shard(x, y)
    for _ in range(5):
        tr.step()
    ref = _torch_run(lambda p: torch.optim.SGD(p, lr=lr, momentum=0.9, weight_decay=1e-4),
                     lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda s: lr_at(s, lr, "cosine", 2, 5, 0.1) / lr),
                     x, y, 128, 5, 1)
    torch.testing.assert_close(tr.params, ref)


# ---- 3. exact resume ----
def _save(tr, step):
    n = tr.n_params
    return ckfmt.decode_full(ckfmt.encode(tr.get_flat().numpy(), {"model": tr.model_name, "step": step},
                                          tr.mom[:n].numpy() if tr.mom is not None else None, tr.state_extra()))


def test_cpu_resume_is_exact_with_adamw_and_warmup():
    x, y = _shard()
    kw = dict(batch=128, lr_warmup_steps=5, **ADAMW)
    a = CPUTrainer(seed=1, **kw)
    a.load_shard(x, y)
    for _ in range(3):
        a.step()
    meta, params, mom, extra = _save(a, 3)
    assert {"cursor", "opt_step", "exp_avg_sq"} == set(extra)
    for _ in range(4):
        a.step()
    b = CPUTrainer(seed=9, **kw)
    b.load_shard(x, y)
    b.set_flat(torch.from_numpy(params))
    b.mom.copy_(torch.from_numpy(mom))
    b.load_state_extra(extra)
    for _ in range(4):
        b.step()
    assert torch.equal(a.params, b.params) and torch.equal(a.mom, b.mom) and torch.equal(a.v, b.v)
    assert torch.equal(a.opt_step, b.opt_step) and int(b.opt_step[0]) == 7


def test_default_trainers_keep_their_state_keys_and_buffers():
    tr = CPUTrainer(batch=128)
    assert set(tr.state_extra()) == {"cursor"} and tr.buffers() == []
    assert tr.v is None and tr.opt_step is None
    assert CPUTrainer(batch=128, momentum=0.0).mom is None
    # AdamW: both moments exist whatever momentum is, and travel with a regroup's broadcast
    ad = CPUTrainer(batch=128, momentum=0.0, **ADAMW)
    assert ad.mom is not None
    assert any(t is ad.v for t in ad.buffers()) and any(t is ad.opt_step for t in ad.buffers())
    sg = CPUTrainer(batch=128, lr_warmup_steps=3)
    assert sg.v is None and [t is sg.opt_step for t in sg.buffers()] == [True]


def test_cpu_resnet_trainer_takes_the_optimizer_arguments():
    from serverless_learn_amd.data.synthetic import make_cifar_like

    x, y = make_cifar_like(8, seed=1)
    tr = make_trainer("resnet18", torch.device("cpu"), batch=4, lr_schedule="linear", lr_warmup_steps=1,
                      lr_decay_steps=4, **ADAMW)
    tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
    w0 = tr.get_flat()
    tr.step()
    assert int(tr.opt_step[0]) == 1 and float(tr.v.abs().sum()) > 0
    assert {"opt_step", "exp_avg_sq"} <= set(tr.state_extra())
    assert tr.buffers()[-2] is tr.v and tr.buffers()[-1] is tr.opt_step
    # the first AdamW step moves every parameter with a gradient by about lr_t = lr (warm-up of 1)
    assert float((tr.get_flat() - w0).abs().max()) == pytest.approx(1e-3, rel=0.05)


# ---- 4. Config / CLI / worker wiring ----
def test_config_cli_and_environment(monkeypatch):
    import argparse

    from serverless_learn_amd.config import Config, add_cli_args, from_args

    ap = argparse.ArgumentParser()
    add_cli_args(ap)
    cfg = from_args(ap.parse_args(["--optimizer", "adamw", "--lr-schedule", "cosine", "--lr-warmup-steps", "5",
                                   "--beta2", "0.95", "--lr-min-ratio", "0.1"]))
    assert (cfg.optimizer, cfg.lr_schedule, cfg.lr_warmup_steps, cfg.beta2, cfg.lr_min_ratio) == (
        "adamw", "cosine", 5, 0.95, 0.1)
    assert (cfg.beta1, cfg.adam_eps, cfg.lr_decay_steps) == (0.9, 1e-8, 0)
    d = Config()
    assert (d.optimizer, d.lr_schedule, d.lr_warmup_steps) == ("sgd", "constant", 0)
    monkeypatch.setenv("SL_OPTIMIZER", "adamw")
    monkeypatch.setenv("SL_LR_DECAY_STEPS", "40")
    e = Config.from_env()
    assert e.optimizer == "adamw" and e.lr_decay_steps == 40


def test_bad_names_fail_at_trainer_construction():
    with pytest.raises(ValueError, match="adamw"):
        make_trainer("mlp", torch.device("cpu"), batch=128, optimizer="adam")
    with pytest.raises(ValueError, match="cosine"):
        make_trainer("mlp", torch.device("cpu"), batch=128, lr_schedule="exp")
    with pytest.raises(ValueError, match="adamw"):
        make_trainer("resnet18", torch.device("cpu"), batch=4, optimizer="lamb")


def _worker(**kw):
    from serverless_learn_amd.runtime.local_cluster import fast_config
    from serverless_learn_amd.runtime.worker import Worker

    return Worker("127.0.0.1:0", fast_config(batch=128, **kw))


def test_worker_builds_the_trainer_from_config():
    w = _worker(optimizer="adamw", lr_schedule="cosine", lr_warmup_steps=5, max_steps=40, lr_min_ratio=0.1, beta2=0.95)
    w._ensure_trainer()
    o = w.trainer.opt
    assert (o.optimizer, o.lr_schedule, o.lr_warmup_steps, o.lr_decay_steps, o.lr_min_ratio, o.beta2) == (
        "adamw", "cosine", 5, 40, 0.1, 0.95)  # lr_decay_steps = 0 means max_steps
    assert w.trainer.v is not None
    with pytest.raises(ValueError, match="lr_decay_steps"):
        _worker(lr_schedule="linear")._ensure_trainer()  # neither a horizon nor max_steps
    with pytest.raises(ValueError, match="sgd"):
        _worker(optimizer="rmsprop")._ensure_trainer()
    d = _worker()
    d._ensure_trainer()
    assert d.trainer.opt.plain and d.trainer.opt.meta() == {"lr": d.cfg.lr, "momentum": d.cfg.momentum}
    assert w.trainer.opt.meta()["name"] == "adamw" and w.trainer.opt.meta()["schedule"] == "cosine"


# ---- 5. optimizer mismatch on load ----
def test_sgd_checkpoint_into_adamw_worker_leaves_the_optimizer_state_zero(monkeypatch):
    x, y = _shard()
    src = CPUTrainer(batch=128, seed=4)
    src.load_shard(x, y)
    for _ in range(3):
        src.step()
    assert float(src.mom.abs().sum()) > 0
    data = ckfmt.encode(src.get_flat().numpy(), {"model": src.model_name, "step": 3,
                                                 "optimizer": {"lr": 0.05, "momentum": 0.9}},
                        src.mom.numpy(), src.state_extra())
    w = _worker(**ADAMW)
    events = []
    monkeypatch.setattr(w.log, "warn", lambda event, **f: events.append((event, f)))
    w._load_checkpoint(data)
    assert torch.equal(w.trainer.params, src.params) and w.trainer.cursor == 3 and w.step == 3
    assert float(w.trainer.mom.abs().sum()) == 0 and float(w.trainer.v.abs().sum()) == 0
    assert int(w.trainer.opt_step[0]) == 0
    assert events and events[0][0] == "checkpoint_optimizer_mismatch"
    assert events[0][1] == {"ckpt": "sgd", "running": "adamw"}
    # ... and the reverse: Adam's first moment is not SGD's momentum
    ad = CPUTrainer(batch=128, seed=4, **ADAMW)
    ad.load_shard(x, y)
    ad.step()
    data = ckfmt.encode(ad.get_flat().numpy(), {"model": ad.model_name, "step": 1, "optimizer": ad.opt.meta()},
                        ad.mom.numpy(), ad.state_extra())
    s = _worker()
    ev2 = []
    monkeypatch.setattr(s.log, "warn", lambda event, **f: ev2.append(event))
    s._load_checkpoint(data)
    assert torch.equal(s.trainer.params, ad.params) and float(s.trainer.mom.abs().sum()) == 0
    assert ev2 == ["checkpoint_optimizer_mismatch"] and set(s.trainer.state_extra()) == {"cursor"}
    # the same optimizer: the whole state loads
    w2 = _worker(**ADAMW)
    w2._load_checkpoint(data)
    assert torch.equal(w2.trainer.mom, ad.mom) and torch.equal(w2.trainer.v, ad.v) and int(w2.trainer.opt_step[0]) == 1
