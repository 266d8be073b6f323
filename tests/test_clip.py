"""Global-norm gradient clipping on the CPU: the reference ``clip_grad_`` (ops/optim.py) against
torch.nn.utils.clip_grad_norm_, the OptSpec field, the CPU trainers against a hand-written
loop, clip-after-exchange, and the Config / worker / metrics wiring."""
import math

import pytest
import torch

from serverless_learn_amd.data.synthetic import make_cifar_like, make_mnist_like
from serverless_learn_amd.models.mlp import CPUTrainer, reference_grads
from serverless_learn_amd.ops.optim import OptSpec, clip_grad_

ADAMW = dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2)
SGD = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)


def _shard(n=256, seed=3):
    x, y = make_mnist_like(n, seed=seed)
    return torch.from_numpy(x), torch.from_numpy(y)


# ---- 1. the reference ----
@pytest.mark.parametrize("factor", [0.25, 3.0, math.inf])
def test_clip_grad_matches_torch(factor):
    gen = torch.Generator().manual_seed(7)
    g0 = torch.randn(1027, generator=gen, dtype=torch.float64)
    g0[::100] *= 1e3
    max_norm = factor * float(g0.norm())
    p = torch.nn.Parameter(torch.zeros_like(g0))
    p.grad = g0.clone()
    ref_total = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
    g = g0.clone()
    total = clip_grad_(g, max_norm)
    assert total == pytest.approx(ref_total, rel=1e-15)
    torch.testing.assert_close(g, p.grad, rtol=1e-15, atol=0.0)
    if factor > 1:
        assert torch.equal(g, g0)  # never scaled up; inf: measured only
    else:
        assert float(g.norm()) == pytest.approx(max_norm, rel=1e-6)


def test_optspec_refuses_negative_and_nan_and_meta_has_the_key_only_when_on():
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="clip_grad_norm"):
            OptSpec(clip_grad_norm=bad)
    off, on, inf = OptSpec(), OptSpec(clip_grad_norm=0.5), OptSpec(clip_grad_norm=math.inf)
    assert off.clip_grad_norm == 0.0 and not off.clips and on.clips and inf.clips
    # clipping needs no step counter: the rule is unchanged
    assert on.plain and on.rule == off.rule and OptSpec(clip_grad_norm=1.0, **ADAMW).rule == OptSpec(**ADAMW).rule
    assert off.meta() == {"lr": off.lr, "momentum": off.momentum}
    assert on.meta() == {"lr": on.lr, "momentum": on.momentum, "clip_grad_norm": 0.5}
    assert "clip_grad_norm" not in OptSpec(**ADAMW).meta()
    assert OptSpec(clip_grad_norm=2.0, **ADAMW).meta()["clip_grad_norm"] == 2.0


# ---- 2. the CPU trainers against a hand-written loop ----
def _loop(spec, params, grads_of, steps, has_mom=True):
    """reference gradient -> clip_grad_ -> rule, by hand: (params, [norms])."""
    w = params.clone()
    m = torch.zeros_like(w) if has_mom else None
    v = torch.zeros_like(w) if spec.adamw else None
    norms = []
    for k in range(steps):
        g = grads_of(w, k)
        norms.append(clip_grad_(g, spec.clip_grad_norm))
        spec.update(w, m, v, g, k)
    return w, norms


@pytest.mark.parametrize("kw", [SGD, ADAMW], ids=["sgd", "adamw"])
def test_cpu_mlp_trainer_clips_every_step(kw):
    B, steps = 64, 4
    x, y = _shard()
    nb = x.shape[0] // B

    def grads_of(w, k):
        b = k % nb
        return reference_grads(w, x[b * B:(b + 1) * B], y[b * B:(b + 1) * B], 1.0 / B)[2]

    probe = CPUTrainer(batch=B, seed=1)
    first = float(grads_of(probe.params, 0).double().norm())
    max_norm = 0.25 * first
    tr = CPUTrainer(batch=B, seed=1, clip_grad_norm=max_norm, **kw)
    assert tr.grad_norm() is None  # no step yet
    tr.load_shard(x, y)
    ref_w, ref_norms = _loop(tr.opt, probe.params, grads_of, steps)
    for k in range(steps):
        tr.step()
        assert tr.grad_norm() == ref_norms[k]
    assert all(n > max_norm for n in ref_norms) and ref_norms[0] == pytest.approx(first, rel=1e-12)
    assert torch.equal(tr.params, ref_w)
    assert set(tr.state_extra()) == set(CPUTrainer(batch=B, seed=1, **kw).state_extra())
    assert CPUTrainer(batch=B, seed=1, **kw).grad_norm() is None


@pytest.mark.parametrize("kw", [SGD, ADAMW], ids=["sgd", "adamw"])
def test_cpu_resnet_trainer_clips_every_step(kw):
    from serverless_learn_amd.models.resnet import CPUResNetTrainer, ref_grads, running_stats

    B, steps = 4, 2
    xn, yn = make_cifar_like(8, seed=1)
    x, y = torch.from_numpy(xn), torch.from_numpy(yn)
    probe = CPUResNetTrainer(batch=B, seed=2)
    x4 = x.reshape(-1, probe.spec.in_hw, probe.spec.in_hw, 3)
    running = running_stats(probe.spec)

    def grads_of(w, k):
        b = k % 2
        return ref_grads(probe.spec, w, x4[b * B:(b + 1) * B], y[b * B:(b + 1) * B], 1.0 / B, running)[2]

    first = float(grads_of(probe.params, 0).double().norm())
    running = running_stats(probe.spec)  # the probe gradient advanced them: the loop starts fresh
    max_norm = 0.25 * first
    tr = CPUResNetTrainer(batch=B, seed=2, clip_grad_norm=max_norm, **kw)
    tr.load_shard(x, y)
    ref_w, ref_norms = _loop(tr.opt, probe.params, grads_of, steps)
    for k in range(steps):
        tr.step()
        assert tr.grad_norm() == ref_norms[k]
    assert all(n > max_norm for n in ref_norms)
    assert torch.equal(tr.params, ref_w)


def test_clip_runs_after_the_exchange_on_the_same_vector():
    """Two replicas on different shards, a hook that gives both the sum of their gradients: the
    clip sees the summed vector, so the replicas end identical (and different from a replica
    that clipped its own gradient first)."""
    B = 64
    xa, ya = _shard(seed=3)
    xb, yb = _shard(seed=4)
    a = CPUTrainer(batch=B, seed=1, world_size=2, clip_grad_norm=0.05, **SGD)
    b = CPUTrainer(batch=B, seed=1, world_size=2, clip_grad_norm=0.05, **SGD)
    a.load_shard(xa, ya)
    b.load_shard(xb, yb)
    seen = []
    for k in range(3):
        bb = k % (xb.shape[0] // B)
        other = {}
        # each replica's hook adds the peer's gradient of the same step (computed on the peer's
        # parameters, which equal its own)
        other["a"] = reference_grads(a.params, xa[bb * B:(bb + 1) * B], ya[bb * B:(bb + 1) * B], 1.0 / (2 * B))[2]
        other["b"] = reference_grads(b.params, xb[bb * B:(bb + 1) * B], yb[bb * B:(bb + 1) * B], 1.0 / (2 * B))[2]

        def hook_a(g):
            g.add_(other["b"])
            seen.append(g.clone())

        def hook_b(g):
            g.copy_(other["a"] + g)  # the same operands in the same order as hook_a's sum
            seen.append(g.clone())

        a.allreduce, b.allreduce = hook_a, hook_b
        a.step()
        b.step()
        assert torch.equal(seen[-1], seen[-2])  # the hooks hand both the unclipped sum
        assert a.grad_norm() == b.grad_norm() == float(seen[-1].double().norm()) and a.grad_norm() > 0.05
    assert torch.equal(a.params, b.params)


# ---- 3. Config / CLI / worker / metrics ----
def test_config_cli_and_environment(monkeypatch):
    import argparse

    from serverless_learn_amd.config import Config, add_cli_args, from_args

    ap = argparse.ArgumentParser()
    add_cli_args(ap)
    assert Config().clip_grad_norm == 0.0
    assert from_args(ap.parse_args(["--clip-grad-norm", "1.5"])).clip_grad_norm == 1.5
    assert from_args(ap.parse_args(["--clip-grad-norm", "inf"])).clip_grad_norm == math.inf
    monkeypatch.setenv("SL_CLIP_GRAD_NORM", "0.25")
    assert Config.from_env().clip_grad_norm == 0.25
    assert from_args(ap.parse_args([])).clip_grad_norm == 0.25


def _worker(**kw):
    from serverless_learn_amd.runtime.local_cluster import fast_config
    from serverless_learn_amd.runtime.worker import Worker

    return Worker("127.0.0.1:0", fast_config(batch=128, **kw))


def test_worker_passes_the_value_under_any_rule_and_skips_xgmi():
    w = _worker(clip_grad_norm=0.75)  # the default optimizer block
    w._ensure_trainer()
    assert w.trainer.opt.plain and w.trainer.opt.clip_grad_norm == 0.75
    assert w.trainer.opt.meta() == {"lr": w.cfg.lr, "momentum": w.cfg.momentum, "clip_grad_norm": 0.75}
    a = _worker(clip_grad_norm=2.0, **ADAMW)
    a._ensure_trainer()
    assert a.trainer.opt.adamw and a.trainer.opt.clip_grad_norm == 2.0
    d = _worker()
    d._ensure_trainer()
    assert d.trainer.opt.clip_grad_norm == 0.0 and d.trainer.grad_norm() is None
    with pytest.raises(ValueError, match="clip_grad_norm"):
        _worker(clip_grad_norm=-1.0)._ensure_trainer()
    assert w._xgmi_wanted() is False


def test_train_event_sets_the_grad_norm_gauge():
    from serverless_learn_amd.utils import metrics

    m = metrics.Metrics("worker")
    m.observe("info", "train", {"step": 10, "loss": 1.5})
    assert 'sl_grad_norm{role="worker"}' not in m.text()
    m.observe("info", "train", {"step": 20, "loss": 1.4, "grad_norm": 3.25})
    assert 'sl_grad_norm{role="worker"} 3.25' in m.text()
