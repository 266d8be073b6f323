"""The state every trainer shares (serverless_learn_amd/models/trainer_state.py): the checkpoint
keys of ``state_extra()``, the order and identity of ``buffers()`` (what a regroup broadcasts beside
params / mom), ``load_state_extra`` and ``reset_optimizer_state``, on all four trainers.

The key lists and buffer orders below are literals recorded from the commit before the trainers shared
this code, by running the same constructors there: a checkpoint written then must load now, and two
ranks of different builds must broadcast the same tensors in the same order.  Everything is an equality
(of names, of identities, of bits); the only tolerance is none.

Shapes: the MLP at its smallest batch (64, one row block), the ResNet on the CPU at batch 4 and 8 x 8
inputs (the smallest the default ``augment_pad`` of 4 admits), on the GPU at the batch 32 / 32 x 32 the
other ResNet GPU tests use.
"""
import numpy as np
import pytest
import torch

from serverless_learn_amd.data.synthetic import make_cifar_like, make_mnist_like
from serverless_learn_amd.models.mlp import CPUTrainer
from serverless_learn_amd.models.resnet import CPUResNetTrainer

DEV = "cuda:0"
CONFIGS = {
    "sgd": {},
    "adamw-cosine": dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2, lr_schedule="cosine", lr_decay_steps=16),
    "clip-accum": dict(clip_grad_norm=1.0, accum_steps=2),
    "ema": dict(ema_decay=0.5),
}
# ---- recorded from the parent commit ----
OPT_KEYS = {"sgd": [], "adamw-cosine": ["opt_step", "exp_avg_sq"], "clip-accum": [], "ema": ["ema", "ema_step"]}
OPT_BUFFERS = {"sgd": [], "adamw-cosine": ["v", "opt_step"], "clip-accum": [], "ema": ["ema", "ema_step"]}
BN_NAMES = ["stem_bn", "layer1.0.bn1", "layer1.0.bn2", "layer1.1.bn1", "layer1.1.bn2", "layer2.0.bn1",
            "layer2.0.bn2", "layer2.0.down_bn", "layer2.1.bn1", "layer2.1.bn2", "layer3.0.bn1", "layer3.0.bn2",
            "layer3.0.down_bn", "layer3.1.bn1", "layer3.1.bn2", "layer4.0.bn1", "layer4.0.bn2",
            "layer4.0.down_bn", "layer4.1.bn1", "layer4.1.bn2"]
BN_KEYS = [f"bn/{name}/{stat}" for name in BN_NAMES for stat in ("mean", "var")]
# the ticket words each engine's launches use, and the state they exist with
TICKETS = {"gpu-mlp": {"opt_ticket": "opt_step", "ema_ticket": "ema"}, "gpu-resnet": {"ema_ticket": "ema"}}

KINDS = pytest.mark.parametrize("kind", ["cpu-mlp", "cpu-resnet"])
CFGS = pytest.mark.parametrize("cfg", list(CONFIGS))


def _make(kind: str, cfg: str, seed: int = 1):
    """A trainer of ``kind`` under ``CONFIGS[cfg]`` with a shard of two batches loaded."""
    kw = CONFIGS[cfg]
    if kind.endswith("mlp"):
        x, y = make_mnist_like(128, seed=0)
        if kind == "cpu-mlp":
            tr = CPUTrainer(batch=64, seed=seed, **kw)
        else:
            from serverless_learn_amd.models.mlp import FusedMLPTrainer

            tr = FusedMLPTrainer(batch=64, device=DEV, seed=seed, **kw)
    elif kind == "cpu-resnet":
        g = torch.Generator().manual_seed(0)  # (the synthetic CIFAR generator starts at 16 x 16)
        x = torch.randint(0, 256, (8, 8, 8, 3), generator=g, dtype=torch.uint8).numpy()
        y = torch.randint(0, 10, (8,), generator=g, dtype=torch.uint8).numpy()
        tr = CPUResNetTrainer(batch=4, in_hw=8, seed=seed, **kw)
    else:
        from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

        x, y = make_cifar_like(64, seed=0)
        tr = FusedResNetTrainer(batch=32, device=DEV, seed=seed, **kw)
    tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
    return tr


def _check_keys_and_buffers(tr, kind: str, cfg: str) -> None:
    bn = BN_KEYS if kind.endswith("resnet") else []
    assert list(tr.state_extra()) == ["cursor"] + bn + OPT_KEYS[cfg]
    want = [t for name in BN_NAMES for t in tr.running_stats()[name]] if bn else []
    want += [getattr(tr, name) for name in OPT_BUFFERS[cfg]]
    got = tr.buffers()
    assert len(got) == len(want) and all(g is w for g, w in zip(got, want))
    absent = {"v", "opt_step", "ema", "ema_step"} - set(OPT_BUFFERS[cfg])
    assert all(getattr(tr, name) is None for name in absent)


def _same_state(a, b) -> None:
    da, db = a.state_extra(), b.state_extra()
    assert list(da) == list(db)
    for k in da:
        assert da[k].dtype == db[k].dtype == np.float64 and np.array_equal(da[k], db[k]), k
    for ta, tb in zip(a.buffers(), b.buffers()):
        assert ta.dtype == tb.dtype and torch.equal(ta, tb)


@KINDS
@CFGS
def test_cpu_keys_buffers_and_exact_round_trip(kind, cfg):
    a = _make(kind, cfg)
    _check_keys_and_buffers(a, kind, cfg)
    a.step()
    a.step()
    _check_keys_and_buffers(a, kind, cfg)  # (a step replaces no state tensor)
    assert a.cursor == 2 * a.accum_steps and a.samples_per_step == a.batch * a.accum_steps
    assert a.grad_scale == 1.0 / (a.batch * a.accum_steps)
    b = _make(kind, cfg, seed=5)
    b.set_flat(a.get_flat())
    b.load_state_extra(a.state_extra())
    assert b.cursor == a.cursor and isinstance(b.cursor, int)
    _same_state(a, b)
    for t in (a.opt_step, a.ema_step):
        if t is not None:
            assert int(t[0]) == 2 and t.dtype == torch.int32


@KINDS
def test_cpu_checkpoint_without_ema_restarts_the_average(kind):
    a = _make(kind, "ema")
    a.step()
    assert int(a.ema_step[0]) == 1 and not torch.equal(a.ema_flat(), a.get_flat())
    b = _make(kind, "ema", seed=5)
    b.step()
    b.set_flat(a.get_flat())
    d = {k: v for k, v in a.state_extra().items() if k not in ("ema", "ema_step")}
    b.load_state_extra(d)
    assert int(b.ema_step[0]) == 0 and torch.equal(b.ema_flat(), a.get_flat()) and b.cursor == a.cursor
    only_step = dict(d, ema_step=a.state_extra()["ema_step"])  # half of the pair is none of it
    b.step()
    b.set_flat(a.get_flat())
    b.load_state_extra(only_step)
    assert int(b.ema_step[0]) == 0 and torch.equal(b.ema_flat(), a.get_flat())


@KINDS
@CFGS
def test_cpu_reset_optimizer_state(kind, cfg):
    tr = _make(kind, cfg)
    tr.step()
    state = [t for t in (tr.mom, tr.v, tr.opt_step) if t is not None]
    assert tr.mom is not None and all(bool(t.any()) for t in state)  # (so the zeros below mean something)
    ema = None if tr.ema is None else (tr.ema.clone(), tr.ema_step.clone())
    params, cursor = tr.params.clone(), tr.cursor
    tr.reset_optimizer_state()
    assert not any(bool(t.any()) for t in state)
    assert torch.equal(tr.params, params) and tr.cursor == cursor
    if ema is not None:
        assert torch.equal(tr.ema, ema[0]) and torch.equal(tr.ema_step, ema[1]) and int(tr.ema_step[0]) == 1


# ---- the GPU engines: the same keys and order, and state that moves between a model's CPU and GPU trainer ----
def _opt_state(tr) -> dict:
    """The optimizer / EMA state as flat CPU tensors (the real entries, without an engine's padding)."""
    n = tr.n_params
    out = {name: getattr(tr, name).detach().cpu() for name in ("opt_step", "ema_step") if getattr(tr, name) is not None}
    out.update({name: getattr(tr, name)[:n].detach().cpu() for name in ("v", "ema") if getattr(tr, name) is not None})
    return out


def _opt_extra(tr, cfg: str) -> dict:
    d = tr.state_extra()
    return {k: d[k] for k in OPT_KEYS[cfg]}


def _assert_same_opt_state(a, b) -> None:
    sa, sb = _opt_state(a), _opt_state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gpu-mlp", "gpu-resnet"])
@CFGS
def test_gpu_keys_buffers_tickets_and_cpu_gpu_exchange(kind, cfg):
    g = _make(kind, cfg)
    _check_keys_and_buffers(g, kind, cfg)
    tickets = {name: getattr(g, name) for name in ("opt_ticket", "ema_ticket")}
    for name, t in tickets.items():  # a ticket exists exactly where the engine's launch uses one
        state = TICKETS[kind].get(name)
        assert (t is not None) == (state is not None and getattr(g, state) is not None), name
    g.step()  # the one training step of this case
    torch.cuda.synchronize()
    _check_keys_and_buffers(g, kind, cfg)
    assert g.samples_per_step == g.batch * g.accum_steps and g.grad_scale == 1.0 / (g.batch * g.accum_steps)
    assert all(int(t.item()) == 0 for t in tickets.values() if t is not None)
    # GPU -> CPU
    cpu_kind = kind.replace("gpu", "cpu")
    c = _make(cpu_kind, cfg, seed=5)
    c.load_state_extra(_opt_extra(g, cfg))
    _assert_same_opt_state(g, c)
    assert c.cursor == 0  # (no "cursor" key passed: left alone)
    # CPU -> GPU, over tickets a run that died inside a launch left set
    c = _make(cpu_kind, cfg, seed=7)
    c.step()
    c.step()
    for t in tickets.values():
        if t is not None:
            t.fill_(3)
    g.load_state_extra(_opt_extra(c, cfg))
    _assert_same_opt_state(c, g)
    assert all(int(t.item()) == 0 for t in tickets.values() if t is not None)
    assert int(g.cursor.item()) == g.accum_steps
    if g.opt_step is not None:
        assert int(g.opt_step.item()) == 2
    g.reset_optimizer_state()
    assert not any(bool(t.any()) for t in (g.mom, g.v, g.opt_step) if t is not None)
    if g.ema is not None:
        assert torch.equal(g.ema_flat().cpu(), c.ema_flat()) and int(g.ema_step.item()) == 2
