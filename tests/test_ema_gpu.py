"""The weight EMA on the GPU: the kernel (csrc/kernels/elementwise.hip ema_flat_kernel, ops/optim.py
ema_flat) and ``ema_decay`` in both training engines.

The definition (README, "Weight EMA"; ops/optim.py ema_update_ and the CPU trainers in test_ema.py): after
every optimizer update ``e <- e + omd_t * (w - e)`` in fp32 -- subtract, multiply, add, each rounded once,
nothing contracted into an fma -- with ``omd_t`` from the table indexed by a device-resident count of EMA
updates, which the same launch advances.  Each of the three operations is correctly rounded, so torch's
fp32 ``e + omd * (w - e)`` is the reference and everything here is an equality of bits.  The MLP engine is
bit-reproducible in the default build, so its cases run in this process; the ResNet engine's cases run
in one ``SL_DETERMINISTIC=1`` child (scripts/ema_resnet_det.py), as tests/test_accum_gpu.py does.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from serverless_learn_amd.ckpt import format as ckfmt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
G = 2048 * 256 * 4  # one pass of the capped grid
SIZES = (1, 3, 255, 1027, 269_322, G + 6)
PAD = 8  # floats (32 bytes: the views stay 16-byte aligned)
LAUNCHES = 5
D, STEPS, B = 0.5, 12, 256
SGD = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
ADAMW_COS_CLIP = dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2, lr_schedule="cosine", lr_warmup_steps=3,
                      lr_decay_steps=16, clip_grad_norm=0.05)
OPTS = pytest.mark.parametrize("kw", [SGD, ADAMW_COS_CLIP], ids=["sgd", "adamw-cosine-clip"])


def _data(n: int, seed: int = 0) -> torch.Tensor:
    """Normal values, 1 % of the entries scaled by 1e3 (as test_accum_gpu._data)."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed + n))
    g[::100] *= 1e3
    return g


def _tab3() -> torch.Tensor:
    return torch.tensor([0.9, 0.5294118, 1.0 - 0.9999], dtype=torch.float32)


def _counters():
    return torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)


# ---- 1. the kernel ----
@pytest.fixture(scope="module")
def vectors():
    """Per size: (ema, w) contents on the host and the reference after each of the launches; built once."""
    tab, out = _tab3(), {}
    for n in SIZES:
        e, w = _data(n), _data(n, seed=1)
        w[1::7] = e[1::7]  # fixed points among them
        refs = []
        for t in range(LAUNCHES):
            e = e + tab[min(t, 2)] * (w - e)  # torch fp32 on the host: three roundings
            refs.append(e)
        out[n] = (_data(n), w, refs)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_kernel_is_exact_and_counts(vectors, n):
    from serverless_learn_amd.ops import optim as O

    e0, w0, refs = vectors[n]
    ebuf, wbuf = torch.full((n + 2 * PAD,), 7e30), torch.full((n + 2 * PAD,), -3e30)
    ebuf[PAD:PAD + n] = e0
    wbuf[PAD:PAD + n] = w0
    ed, wd, tab = ebuf.to(DEV), wbuf.to(DEV), _tab3().to(DEV)
    ema, w = ed[PAD:PAD + n], wd[PAD:PAD + n]
    assert ema.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
    step, ticket = _counters()
    for t in range(LAUNCHES):
        O.ema_flat(ema, w, step, ticket, tab)
        torch.cuda.synchronize()
        out = ed.cpu()
        got = out[PAD:PAD + n]
        assert torch.equal(got, refs[t]), (n, t, int((got != refs[t]).sum()))
        assert int(step.item()) == t + 1 and int(ticket.item()) == 0, (n, t)
        assert torch.equal(out[:PAD], ebuf[:PAD]) and torch.equal(out[PAD + n:], ebuf[PAD + n:]), (n, t)
    assert torch.equal(wd.cpu(), wbuf)  # the parameters are only read
    fixed = refs[-1][1::7]
    assert torch.equal(fixed, w0[1::7])  # w == e stayed put through every launch


def test_entry_point_refuses_bad_arguments():
    from serverless_learn_amd.ops import _native as N
    from serverless_learn_amd.ops import optim as O

    lib = N.lib()
    e, w, tab = torch.ones(64, device=DEV), torch.full((64,), 3.0, device=DEV), torch.tensor([0.5], device=DEV)
    step, ticket = _counters()
    st = N.stream_ptr()
    args = lambda **k: tuple({**dict(e=e.data_ptr(), w=w.data_ptr(), n=64, s=step.data_ptr(), t=ticket.data_ptr(),  # noqa: E731
                                     tab=tab.data_ptr(), tn=1), **k}.values()) + (st,)
    assert lib.sl_ema_flat(*args()) == 0
    for bad in (dict(e=None), dict(w=None), dict(s=None), dict(t=None), dict(tab=None), dict(tn=0), dict(tn=-1),
                dict(e=e.data_ptr() + 4, n=60), dict(w=w.data_ptr() + 8, n=60)):
        assert lib.sl_ema_flat(*args(**bad)) == -1, bad
    assert lib.sl_ema_flat(*args(n=0)) == 0 and lib.sl_ema_flat(*args(n=-5)) == 0
    torch.cuda.synchronize()
    assert int(step.item()) == 1 and int(ticket.item()) == 0  # one launch ran; n <= 0 left the counter alone
    assert torch.equal(e, torch.full((64,), 2.0, device=DEV)) and float(w.sum()) == 192.0
    with pytest.raises(AssertionError, match="overlap"):
        O.ema_flat(e[:40], e[24:], step, ticket, tab)
    with pytest.raises(AssertionError):
        O.ema_flat(e, w[:32], step, ticket, tab)
    with pytest.raises(AssertionError):
        O.ema_flat(e, w.double(), step, ticket, tab)
    with pytest.raises(AssertionError):
        O.ema_flat(e, w, step.long(), ticket, tab)
    assert O.EMA_KERNELS == ("sl_ema_flat",)


def test_graph_replays_the_kernel_and_its_counter():
    from serverless_learn_amd.ops import optim as O

    n = 5 * 1024 + 3
    tab, w = _tab3().to(DEV), _data(n, seed=1).to(DEV)
    ema, twin = _data(n).to(DEV), _data(n).to(DEV)
    step, ticket = _counters()
    step2, ticket2 = _counters()
    O.ema_flat(ema, w, step, ticket, tab)  # the kernel's code is loaded before the capture
    O.ema_flat(twin, w, step2, ticket2, tab)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        O.ema_flat(ema, w, step, ticket, tab)
    for _ in range(LAUNCHES):
        graph.replay()
        O.ema_flat(twin, w, step2, ticket2, tab)
    torch.cuda.synchronize()
    assert torch.equal(ema, twin) and int(step.item()) == int(step2.item()) == 1 + LAUNCHES
    assert int(ticket.item()) == 0
    want = _data(n)
    for t in range(1 + LAUNCHES):  # the coefficient moved inside the graph: 0.9, 0.529, then the last
        want = want + _tab3()[min(t, 2)] * (w.cpu() - want)
    assert torch.equal(ema.cpu(), want)


# ---- 2. the MLP engine ----
def _mnist(batches: int, batch: int):
    from serverless_learn_amd.data.synthetic import make_mnist_like

    x, y = make_mnist_like(batches * batch, seed=3)
    return torch.from_numpy(x), torch.from_numpy(y)


@pytest.fixture(scope="module")
def shard():
    return _mnist(4, B)


def _mlp(shard, seed=1, **kw):
    from serverless_learn_amd.models.mlp import FusedMLPTrainer

    tr = FusedMLPTrainer(batch=B, device=DEV, seed=seed, **kw)
    tr.load_shard(*shard)
    return tr


TRAINING = ("params", "mom", "v", "w1h", "w2h", "w2th", "w3h", "w3th", "r1p", "opt_step", "opt_ticket", "cursor",
            "grad", "loss", "correct", "clip_norm")
AVERAGE = ("ema", "ema_step", "ema_ticket")


def _same_trainers(a, b, what, names=TRAINING):
    """Bit-identical: parameters, both moments, every shadow, the W1 row sums and the counters."""
    for name in names:
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None), (what, name)
        if ta is not None:
            assert torch.equal(ta, tb), (what, name, int((ta != tb).sum()))


def _follow(tr, steps, e, tab, t0=0):
    """``steps`` steps; after each, ema_flat() against the recurrence over the get_flat() snapshots."""
    for t in range(t0, t0 + steps):
        tr.step()
        w = tr.get_flat().cpu()
        e = e + tab[min(t, tab.numel() - 1)] * (w - e)
        assert torch.equal(tr.ema_flat().cpu(), e), (t, int((tr.ema_flat().cpu() != e).sum()))
        assert int(tr.ema_step.item()) == t + 1 and int(tr.ema_ticket.item()) == 0
    return e


@pytest.fixture(scope="module")
def eager(shard):
    """Per optimizer: the EMA trainer after 12 eager steps under the recurrence, and its EMA-off twin."""
    from serverless_learn_amd.ops import optim as O

    out = {}
    for name, kw in (("sgd", SGD), ("adamw-cosine-clip", ADAMW_COS_CLIP)):
        tr, twin = _mlp(shard, ema_decay=D, **kw), _mlp(shard, **kw)
        tab = torch.from_numpy(O.ema_table(D, True))
        assert torch.equal(tr.ema_tab.cpu(), tab) and tab.numel() == 9
        assert torch.equal(tr.ema_flat(), tr.get_flat()) and tr.ema.shape == tr.params.shape
        _follow(tr, STEPS, tr.get_flat().cpu(), tab)  # passes the saturation at t = 8
        for _ in range(STEPS):
            twin.step()
        torch.cuda.synchronize()
        out[name] = (tr, twin)
    return out


@OPTS
def test_mlp_follows_the_recurrence_and_trains_like_the_twin(eager, kw, request):
    tr, twin = eager[request.node.callspec.id]
    _same_trainers(tr, twin, "EMA on vs off")
    assert not torch.equal(tr.ema, tr.params) and int(tr.cursor.item()) == STEPS
    assert twin.ema is None and twin.ema_step is None and twin.ema_ticket is None and twin.ema_tab is None
    assert twin._ema_eval is None and tr._ema_eval is None
    assert "ema" in tr._launches() and "ema" not in twin._launches()
    assert sorted(set(tr.state_extra()) - set(twin.state_extra())) == ["ema", "ema_step"]
    assert len(tr.buffers()) == len(twin.buffers()) + 2
    assert tr.buffers()[-2] is tr.ema and tr.buffers()[-1] is tr.ema_step


def test_ema_off_launches_and_state_are_what_they_were(shard):
    off = _mlp(shard, **SGD)
    assert set(off._launches()) == {"rows", "wgrad", "sgd", "reduce", "update"}
    assert sorted(off.state_extra()) == ["cursor"] and off.buffers() == []
    on = _mlp(shard, ema_decay=D, ema_warmup=False, **SGD)
    assert set(on._launches()) == {"rows", "wgrad", "sgd", "reduce", "update", "ema"} and on.ema_tab.numel() == 1
    key = on._lkey
    on.set_optimizer(ema_decay=0.9)  # the settings are in the key: the launches are rebuilt
    assert on._launches() and on._lkey != key and float(on.ema_tab[0]) == pytest.approx(0.1)
    with pytest.raises(ValueError, match="construction"):
        on.set_optimizer(ema_decay=0.0)
    with pytest.raises(ValueError, match="construction"):
        off.set_optimizer(ema_decay=0.5)

    class Exchange:
        payload_floats = 1 << 20
        two_shot = inline_sync = False

    on.enable_xgmi(Exchange())  # the EMA is local: the xGMI exchange keeps accepting such a trainer
    on.enable_xgmi(None)
    from serverless_learn_amd.models.mlp import FusedMLPTrainer

    for bad in (-0.1, float("nan"), 1.0):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedMLPTrainer(batch=64, device=DEV, ema_decay=bad)
    with pytest.raises(ValueError, match="ema_warmup off"):
        FusedMLPTrainer(batch=64, device=DEV, ema_decay=1.0 - 1e-7)


@OPTS
def test_mlp_captured_graphs_equal_eager(eager, shard, kw, request):
    e = eager[request.node.callspec.id][0]
    for unroll in (1, 4):
        a = _mlp(shard, ema_decay=D, **kw)
        a.capture(warmup=0, unroll=unroll)
        a.steps(STEPS)
        torch.cuda.synchronize()
        _same_trainers(a, e, f"graph unroll={unroll} vs eager", TRAINING + AVERAGE)
        assert int(a.ema_step.item()) == STEPS and int(a.ema_ticket.item()) == 0
        a.drop_graphs()


def test_mlp_one_update_per_accumulated_step(shard):
    from serverless_learn_amd.ops import optim as O

    tr, twin = _mlp(shard, ema_decay=D, accum_steps=2, **SGD), _mlp(shard, accum_steps=2, **SGD)
    _follow(tr, STEPS, tr.get_flat().cpu(), torch.from_numpy(O.ema_table(D, True)))
    for _ in range(STEPS):
        twin.step()
    torch.cuda.synchronize()
    assert int(tr.ema_step.item()) == STEPS and int(tr.cursor.item()) == 2 * STEPS
    _same_trainers(tr, twin, "accumulated, EMA on vs off")
    g = _mlp(shard, ema_decay=D, accum_steps=2, **SGD)
    g.capture(warmup=0, unroll=4)
    g.steps(STEPS)
    torch.cuda.synchronize()
    _same_trainers(g, tr, "accumulated graph vs eager", TRAINING + AVERAGE)
    g.drop_graphs()


# ---- 3. evaluation ----
def _snapshot(tr):
    names = [n for n in TRAINING + AVERAGE if getattr(tr, n) is not None]
    return {n: getattr(tr, n).clone() for n in names}, {n: getattr(tr, n).data_ptr() for n in names}


def test_mlp_evaluates_the_average_and_leaves_training_alone(shard):
    from serverless_learn_amd.models.mlp import FusedMLPTrainer

    x, y = _mnist(3, B)
    tr, twin = _mlp(shard, ema_decay=D, **ADAMW_COS_CLIP), _mlp(shard, ema_decay=D, **ADAMW_COS_CLIP)
    for t in (tr, twin):
        t.capture(warmup=0, unroll=4)
        t.steps(5)
    torch.cuda.synchronize()
    before, ptrs = _snapshot(tr)
    avg, own = tr.evaluate(x, y, ema=True), tr.evaluate(x, y)
    la, lo = tr.logits(x, ema=True), tr.logits(x)
    torch.cuda.synchronize()
    second = FusedMLPTrainer(batch=B, device=DEV, seed=8, flat=tr.ema_flat())
    want = second.evaluate(x, y)
    assert (avg.loss, avg.accuracy, avg.n) == (want.loss, want.accuracy, want.n) and avg.n == 3 * B
    assert torch.equal(la, second.logits(x))
    assert avg.loss != own.loss and not torch.equal(la, lo)
    plain = FusedMLPTrainer(batch=B, device=DEV, seed=8, flat=tr.get_flat())
    assert own.loss == plain.evaluate(x, y).loss and torch.equal(lo, plain.logits(x))  # ema=False is what it was
    after, ptrs_after = _snapshot(tr)
    assert ptrs == ptrs_after and tr.graph is not None and tr.graph_unrolled is not None  # no tensor moved
    for name in before:
        assert torch.equal(before[name], after[name]), name
    # the shadows of the average are its own set, what the second trainer holds
    for name in ("w1h", "w2h", "w2th", "w3h", "w3th", "r1p"):
        assert torch.equal(tr._ema_eval[name], getattr(second, name)), name
        assert tr._ema_eval[name].data_ptr() != getattr(tr, name).data_ptr()
    # graph replays after the evaluation match the twin that never evaluated
    for t in (tr, twin):
        t.steps(7)
    torch.cuda.synchronize()
    _same_trainers(tr, twin, "replays after evaluate(ema=True)", TRAINING + AVERAGE)
    assert tr.evaluate(x, y, ema=True).loss != avg.loss  # rebuilt from the average as it is now
    for t in (tr, twin):
        t.drop_graphs()
    off = _mlp(shard, **SGD)
    with pytest.raises(ValueError, match="ema"):
        off.evaluate(x, y, ema=True)
    with pytest.raises(ValueError, match="ema"):
        off.logits(x, ema=True)
    with pytest.raises(ValueError, match="ema"):
        off.ema_flat()


# ---- 4. resume ----
def test_mlp_resume_is_bit_exact(shard):
    kw = dict(ema_decay=D, **ADAMW_COS_CLIP)
    a = _mlp(shard, **kw)
    for _ in range(5):
        a.step()
    n = a.n_params
    buf = ckfmt.encode(a.get_flat().cpu().numpy(), {"model": a.model_name, "step": 5}, a.mom[:n].cpu().numpy(),
                       a.state_extra())
    meta, params, mom, extra = ckfmt.decode_full(buf)
    assert int(extra["ema_step"][0]) == 5 and extra["ema"].size == n
    b = _mlp(shard, seed=99, **kw)  # another init: everything must come from the file
    assert not torch.equal(b.ema, a.ema)
    b.ema_ticket.fill_(3)  # (as a run that died inside the launch would leave it)
    b.set_flat(torch.from_numpy(params))
    b.mom[:n].copy_(torch.from_numpy(mom))
    b.load_state_extra(extra)
    assert torch.equal(b.ema, a.ema) and int(b.ema_ticket.item()) == 0
    for _ in range(5):
        a.step()
        b.step()
    torch.cuda.synchronize()
    _same_trainers(a, b, "resumed vs straight", TRAINING + AVERAGE)
    assert int(a.ema_step.item()) == 10
    # a file without the keys: the average starts over from the loaded weights
    b.load_state_extra({k: v for k, v in extra.items() if k not in ("ema", "ema_step")})
    assert torch.equal(b.ema, b.params) and int(b.ema_step.item()) == 0
    # an EMA file into a trainer without one: ignored
    c = _mlp(shard, seed=99, **ADAMW_COS_CLIP)
    c.load_state_extra(extra)
    assert c.ema is None and int(c.cursor.item()) == 5
    # set_flat, refresh_shadows and reset_optimizer_state leave the average alone
    e = a.ema_flat()
    a.set_flat(b.get_flat())
    a.refresh_shadows()
    a.reset_optimizer_state()
    assert torch.equal(a.ema_flat(), e) and int(a.ema_step.item()) == 10


# ---- the runtime worker ----
def test_worker_trains_with_the_ema_from_graph_chunks():
    """A worker with ema_decay set runs its steps from captured chunks and ends bit-identical, the
    average included, to the bare engine stepped eagerly on the same shard."""
    from serverless_learn_amd.models.mlp import FusedMLPTrainer
    from serverless_learn_amd.runtime.local_cluster import LocalCluster, fast_config

    steps = 24
    c = LocalCluster(fast_config(device=DEV, batch=B, shard_records=8 * B, log_every=8, graph_steps=4, ema_decay=D,
                                 max_steps=steps))
    try:
        w = c.add_worker(sync="none")
        assert c.wait_for(lambda: w.state == "done", 60), (w.state, w.step)
        torch.cuda.synchronize()
        t = w.trainer
        assert w.step == steps and w.graph_chunks > 0 and int(t.ema_step.item()) == steps
        eng = FusedMLPTrainer(batch=B, device=DEV, ema_decay=D)
        eng.load_shard(t.x, t.y)
        for _ in range(steps):
            eng.step()
        torch.cuda.synchronize()
        _same_trainers(t, eng, "worker vs bare engine", ("params", "mom", "w1h", "w2h", "w2th", "w3h", "w3th", "r1p",
                                                         "cursor") + AVERAGE)
        assert not torch.equal(t.ema, t.params)
    finally:
        c.stop()


# ---- 5. the ResNet engine, in one deterministic-build child ----
@pytest.fixture(scope="module")
def resnet_child():
    env = dict(os.environ, SL_DETERMINISTIC="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "ema_resnet_det.py")], env=env,
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["deterministic_build"], r
    return r


def test_resnet_follows_the_recurrence_and_trains_like_the_twin(resnet_child):
    r = resnet_child["eager"]
    print(r)
    assert r["finite"] and r["starts_at_params"] and r["table"] == 9 and r["twin_has_no_ema"], r
    assert r["recurrence"] == [True] * 6 and r["ema_step"] == 6 and r["ticket"] == 0, r
    assert r["ema_differs_from_params"], r
    assert r["params_identical"] and r["mom_identical"] and r["shadow_identical"], r
    assert r["running_stats_identical"] and r["cursor"] == [6, 6], r


def test_resnet_captured_graph_follows_the_recurrence(resnet_child):
    r = resnet_child["graph"]
    print(r)
    assert r["captured"] and r["after_warmup_identical"] and r["recurrence"] == [True] * 4, r
    assert r["ema_step"] == 6 and r["ticket"] == 0, r
    assert r["ema_identical_to_eager"] and r["params_identical_to_eager"] and r["mom_identical_to_eager"], r
    assert r["running_stats_identical"], r


def test_resnet_evaluates_the_average_and_leaves_training_alone(resnet_child):
    r = resnet_child["evaluate"]
    print(r)
    assert r["equals_second_trainer"] and r["differs_from_params"] and r["n"] == 192, r
    assert r["state_identical"] and r["state_tensors"] > 60 and r["no_tensor_moved"], r
    assert r["raises_without_ema"] and r["next_step_equals_twin"] and r["next_replay_equals_eager"], r


def test_resnet_resume_is_bit_exact(resnet_child):
    r = resnet_child["resume"]
    print(r)
    assert r["fresh_trainer_differs"] and r["loaded_identical"], r
    assert r["ema_identical"] and r["params_identical"] and r["mom_identical"] and r["v_identical"], r
    assert r["running_stats_identical"] and r["ema_step"] == [6, 6] and r["ckpt_ema_step"] == 3, r
    assert r["ckpt_ema_size"] == r["n_params"] and r["without_keys_from_weights"], r


def test_resnet_buffers_and_state_keys(resnet_child):
    r = resnet_child["eager"]
    assert r["buffers_extra"] == 2 and r["buffers_carry_ema"], r
    assert r["state_keys_extra"] == ["ema", "ema_step"] and r["twin_state_keys_as_before"], r
