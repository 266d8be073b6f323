"""Gradient accumulation on the CPU: the configuration, the CPU trainers (the definition the GPU
engines are tested against in test_accum_gpu.py), the worker's nearest-K rule for a requested
global batch, and a two-process gloo group.

One step of ``accum_steps = K`` at batch cursor ``t`` runs micro-batches at cursors ``t .. t + K - 1``
with ``grad_scale = 1 / (batch * world * K)`` and applies ``((g_0 + g_1) + g_2) + ...``, summed in fp32
in that order, through one exchange, one clip and one update.
"""
import argparse
import socket

import pytest
import torch
import torch.multiprocessing as mp

from serverless_learn_amd.config import Config, add_cli_args, from_args
from serverless_learn_amd.data.synthetic import make_cifar_like, make_mnist_like
from serverless_learn_amd.models import make_trainer
from serverless_learn_amd.models import mlp as M
from serverless_learn_amd.models import resnet as R

K = 3


# ---- configuration ----
def test_config_accepts_and_refuses():
    assert (Config().accum_steps, Config().global_batch) == (1, 0)
    assert Config(accum_steps=4).accum_for(3) == 4
    assert Config(batch=64, global_batch=64).accum_for(1) == 1
    Config(batch=64, global_batch=1000, model="resnet18")
    for bad in (dict(accum_steps=0), dict(accum_steps=-2), dict(accum_steps=2, global_batch=4096),
                dict(batch=64, global_batch=63), dict(batch=64, global_batch=1), dict(global_batch=-1),
                dict(accum_steps=2, model="simulate"), dict(global_batch=4096, model="simulate")):
        with pytest.raises(ValueError):
            Config(**bad)
    cfg = Config()
    cfg.accum_steps = 0  # set after construction: the worker validates again
    with pytest.raises(ValueError):
        cfg.validate()


def test_cli_flags_and_environment_round_trip(monkeypatch):
    ap = argparse.ArgumentParser()
    add_cli_args(ap)
    assert from_args(ap.parse_args(["--accum-steps", "4"])).accum_steps == 4
    cfg = from_args(ap.parse_args(["--global-batch", "8192", "--batch", "1024"]))
    assert (cfg.global_batch, cfg.accum_steps, cfg.accum_for(2)) == (8192, 1, 4)
    monkeypatch.setenv("SL_ACCUM_STEPS", "3")
    assert Config.from_env().accum_steps == 3
    assert from_args(ap.parse_args([])).accum_steps == 3
    assert from_args(ap.parse_args(["--accum-steps", "2"])).accum_steps == 2  # the flag wins
    monkeypatch.delenv("SL_ACCUM_STEPS")
    monkeypatch.setenv("SL_GLOBAL_BATCH", "2048")
    assert Config.from_env().global_batch == 2048
    monkeypatch.setenv("SL_ACCUM_STEPS", "2")
    with pytest.raises(ValueError):
        Config.from_env()


def test_nearest_k_rule():
    cfg = Config(batch=64, global_batch=256)
    assert [cfg.accum_for(w) for w in (1, 2, 3, 4, 5)] == [4, 2, 1, 1, 1]
    # floor(G / (batch * world) + 1/2): a tie rounds up
    assert Config(batch=64, global_batch=96).accum_for(1) == 2 and Config(batch=64, global_batch=95).accum_for(1) == 1


# ---- the CPU trainers ----
def _ordered_sum(grads):
    g = grads[0]
    for gi in grads[1:]:
        g = g + gi
    return g


@pytest.mark.parametrize("opt", [dict(lr=0.1, momentum=0.9), dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2)],
                         ids=["sgd", "adamw"])
def test_cpu_mlp_trainer_accumulates_in_order(opt):
    B = 32
    x, y = make_mnist_like(4 * B, seed=2)
    x, y = torch.from_numpy(x), torch.from_numpy(y)
    tr = M.CPUMLPTrainer(batch=B, seed=1, accum_steps=K, **opt)
    assert M.CPUMLPTrainer is M.CPUTrainer and tr.samples_per_step == K * B and tr.grad_scale == 1.0 / (K * B)
    tr.load_shard(x, y)
    tr.cursor = 2  # micro-batches 2, 3 and (wrapping) 0
    w0 = tr.params.clone()
    tr.step()
    parts = [M.reference_grads(w0, x[b * B:(b + 1) * B], y[b * B:(b + 1) * B], 1.0 / (K * B)) for b in (2, 3, 0)]
    g = _ordered_sum([p[2] for p in parts])
    assert g.dtype == torch.float32 and torch.equal(tr.grad, g)
    assert not torch.equal(g, _ordered_sum([p[2] for p in reversed(parts)]))  # the order is observable
    # one update with that gradient
    twin = M.CPUTrainer(batch=B, flat=w0, **opt)
    twin._opt_update(g.clone())
    assert torch.equal(tr.params, twin.params) and torch.equal(tr.mom, twin.mom)
    assert tr.cursor == 2 + K
    if tr.opt_step is not None:
        assert int(tr.opt_step[0]) == 1
    st = tr.stats()
    assert st.n == st.samples == K * B
    assert st.loss == pytest.approx(float(sum(p[0] for p in parts)) / (K * B), rel=1e-6)
    assert st.accuracy == pytest.approx(float(sum(p[1] for p in parts)) / (K * B))


def test_cpu_resnet_trainer_accumulates_in_order():
    B = 4
    x, y = make_cifar_like(K * B, seed=3)
    x, y = torch.from_numpy(x), torch.from_numpy(y)
    tr = R.CPUResNetTrainer(batch=B, seed=5, accum_steps=K, optimizer="adamw", lr=1e-3)
    tr.load_shard(x, y)
    w0 = tr.params.clone()
    tr.step()
    running = R.running_stats(tr.spec)  # updated once per micro-batch, as torch does under accumulation
    xs = x.reshape(-1, 32, 32, 3)
    parts = [R.ref_grads(tr.spec, w0, xs[b * B:(b + 1) * B], y[b * B:(b + 1) * B], 1.0 / (K * B), running)
             for b in range(K)]
    assert torch.equal(tr.grad, _ordered_sum([p[2] for p in parts]))
    for name, (rm, rv) in running.items():
        assert torch.equal(rm, tr.running[name][0]) and torch.equal(rv, tr.running[name][1]), name
    assert tr.cursor == K and int(tr.opt_step[0]) == 1 and tr.stats().n == K * B
    assert tr.stats().loss == pytest.approx(float(sum(p[0] for p in parts)) / (K * B), rel=1e-6)
    assert not torch.equal(tr.params, w0)


def test_k1_trainers_are_as_before_and_bad_k_raises():
    for tr in (make_trainer("mlp", torch.device("cpu"), batch=8), make_trainer("resnet18", torch.device("cpu"), batch=4)):
        assert tr.accum_steps == 1 and tr.samples_per_step == tr.batch
    assert make_trainer("mlp", torch.device("cpu"), batch=8, accum_steps=2).samples_per_step == 16
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            M.CPUTrainer(batch=8, accum_steps=bad)
    tr = M.CPUTrainer(batch=8, world_size=2)
    tr.set_accum(4)
    tr.set_world(4)
    assert tr.grad_scale == 1.0 / (8 * 4 * 4)


# ---- the worker ----
def test_worker_keeps_the_global_batch_across_regroups():
    from serverless_learn_amd.runtime.worker import Worker

    B = 64
    cfg = Config(device="cpu", model="mlp", batch=B, global_batch=256, sync="allreduce", graph=False, max_steps=1,
                 log_every=1)
    w = Worker("localhost:0", cfg)
    events = []
    info = w.log.info
    w.log.info = lambda event, **f: (events.append((event, f)), info(event, **f))[1]
    try:
        w.view = dict(w.view, world=4)
        w._ensure_trainer()
        t = w.trainer
        assert (t.accum_steps, t.world_size, t.grad_scale) == (1, 4, 1.0 / 256)
        w._set_world(2)
        assert (t.accum_steps, t.grad_scale) == (2, 1.0 / 256)
        w._set_world(3)  # nearest: 1 x 64 x 3 = 192; the scale is the batch actually reached
        assert (t.accum_steps, t.grad_scale) == (1, 1.0 / 192)
        w._set_world(1)
        assert (t.accum_steps, t.grad_scale, t.samples_per_step) == (4, 1.0 / 256, 256)
        assert [f["accum_steps"] for e, f in events if e == "accum_steps"] == [2, 1, 4]
        # one step of the training loop: the train event and the gauge report the batch reached
        w.view = dict(w.view, world=0)
        x, y = make_mnist_like(4 * B, seed=0)
        w._pending_shard = (torch.from_numpy(x), torch.from_numpy(y), 1)
        w._train_loop()
        train = [f for e, f in events if e == "train"]
        assert len(train) == 1 and train[0]["global_batch"] == 256 and train[0]["accum_steps"] == 4
        assert (w.step, w.samples, t.cursor) == (1, 256, 4)
        if w.metrics.enabled:
            assert 'sl_global_batch{role="worker"} 256.0' in w.metrics.text()
    finally:
        w.channels.close()


# ---- a gloo group ----
STEPS, BATCH, WORLD, KG = 3, 64, 2, 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _group_data():
    x, y = make_mnist_like(STEPS * WORLD * KG * BATCH, seed=1)
    return torch.from_numpy(x), torch.from_numpy(y)


def _rank_main(rank, port, out_path):
    import torch.distributed as dist

    from serverless_learn_amd.parallel.dp import ElasticGroup

    if rank == 0:
        store = dist.TCPStore("127.0.0.1", port, is_master=True, wait_for_workers=False)  # noqa: F841
    g = ElasticGroup(device=torch.device("cpu"), timeout_s=30)
    assert g.reform(1, rank, WORLD, f"127.0.0.1:{port}")
    x, y = _group_data()
    x = x.view(STEPS, WORLD, KG, BATCH, -1)[:, rank].reshape(-1, 784)
    y = y.view(STEPS, WORLD, KG, BATCH)[:, rank].reshape(-1)
    tr = M.CPUTrainer(batch=BATCH, lr=0.1, momentum=0.9, world_size=WORLD, seed=3, accum_steps=KG)
    tr.load_shard(x, y)
    calls = []
    tr.allreduce = lambda t: (calls.append(1), g.allreduce_(t))[1]
    for _ in range(STEPS):
        tr.step()
    assert len(calls) == STEPS  # one exchange per step, not per micro-batch
    torch.save(tr.params, out_path)
    g.teardown()


@pytest.mark.slow
def test_gloo_group_with_accumulation_matches_one_trainer(tmp_path):
    port = _free_port()
    outs = [str(tmp_path / f"r{r}.pt") for r in range(WORLD)]
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_main, args=(r, port, outs[r])) for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    p0, p1 = (torch.load(o, weights_only=True) for o in outs)
    assert torch.equal(p0, p1)
    # one trainer fed the same four micro-batches per step in rank-major order: the same global
    # batch and gradient scale, 1 / (4 * BATCH); the tolerance is test_dp_multiprocess.py's
    x, y = _group_data()
    ref = M.CPUTrainer(batch=BATCH, lr=0.1, momentum=0.9, seed=3, accum_steps=WORLD * KG)
    ref.load_shard(x, y)
    for _ in range(STEPS):
        ref.step()
    assert ref.cursor == STEPS * WORLD * KG
    assert torch.allclose(p0, ref.params, atol=3e-4, rtol=1e-3), (p0 - ref.params).abs().max()
