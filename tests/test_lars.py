"""LARS on the CPU: the plan (ops/optim.py lars_plan), the reference update against a per-tensor loop, the CPU
ResNet trainer, the refusals and the flags.  test_lars_gpu.py uses the synthetic layout and state built here."""
import math

import numpy as np
import pytest
import torch

from serverless_learn_amd.config import Config
from serverless_learn_amd.ops.optim import DECAY_BLOCK, LARS_CHUNK, LARS_NO_TENSOR, OptSpec, lars_plan, lars_update

C = LARS_CHUNK
# one block; exactly one chunk; a norm pair; a ragged second chunk (6: a float4 and a 2-element tail); a bias; four
# chunks, the last of 70; a tensor that is no multiple of 4, which ends the vector unpadded (n % 4 == 2)
SIZES = (("a.weight", 64), ("b.weight", C), ("n.weight", 10), ("n.bias", 10), ("c.weight", C + 6), ("h.bias", 10),
         ("d.weight", 3 * C + 70), ("e.weight", 130))
NORM = ("n.weight", "n.bias")
ADAPTED = ("a.weight", "b.weight", "c.weight", "d.weight", "e.weight")
DECAYS = (5e-4, 0.0, 1e-4)
ETA, EPS = 0.02, 1e-9


def synthetic(sizes=SIZES):
    """(layout, n): the tensors of ``sizes`` in order, each on a 64-element boundary; the last one ends the vector."""
    layout, off = [], 0
    for name, numel in sizes:
        layout.append([name, [numel], off])
        n, off = off + numel, off + (numel + DECAY_BLOCK - 1) // DECAY_BLOCK * DECAY_BLOCK
    return layout, n


def state(layout, n, seed=0):
    """Seeded fp32 (w, g, mom), zero in the padding; ``a.weight`` has a zero gradient and ``e.weight`` zero weights."""
    gen = torch.Generator().manual_seed(seed)
    w, g, m = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    for name, (numel,), off in layout:
        for t, scale in ((w, 0.0 if name == "e.weight" else 0.1), (g, 0.0 if name == "a.weight" else 0.01), (m, 0.01)):
            t[off:off + numel] = torch.randn(numel, generator=gen) * scale
    return w, g, m


def test_plan_tiles_every_adapted_tensor():
    layout, n = synthetic()
    p = lars_plan(layout, n, NORM)
    assert p.names == ADAPTED and p.n == n and p.chunks.dtype == np.int32 and p.block_map.dtype == np.uint16
    by_name = {name: (off, numel) for name, (numel,), off in layout}
    owner, cls, nxt = np.repeat(p.block_map, DECAY_BLOCK)[:n], np.repeat(p.cls, DECAY_BLOCK)[:n], 0
    for t, (name, (off, numel, first, count)) in enumerate(zip(p.names, p.tensors.tolist())):
        assert (off, numel) == by_name[name] and first == nxt and count == -(-numel // C)
        at = off
        for k, (o, c) in enumerate(p.chunks[first:first + count].tolist()):
            assert o == at and o % 4 == 0 and 1 <= c <= C and (c % 4 == 0 or k == count - 1)
            at += c
        assert at == off + numel  # the chunks tile the real elements exactly: none straddles, none is in the padding
        assert (owner[off:off + numel] == t).all()
        nxt += count
    assert nxt == len(p.chunks) and ((owner == LARS_NO_TENSOR) == (cls != 0)).all()


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_lars_update_matches_a_per_tensor_loop(momentum):
    layout, n = synthetic()
    w0, g, m0 = state(layout, n)
    lr, w, m = 0.3, w0.clone(), m0.clone() if momentum else None
    rows = dict(zip(ADAPTED, lars_update(w, m, g, lr, momentum, DECAYS, lars_plan(layout, n, NORM), ETA, EPS)))
    for name, (numel,), off in layout:
        sl = slice(off, off + numel)
        ws, gs, ms = w0[sl].double(), g[sl].double(), m0[sl].double()
        c, trust = 1 if name in NORM else 2 if name.endswith(".bias") else 0, 1.0
        if c == 0:
            wn, gn = math.sqrt(float((ws * ws).sum())), math.sqrt(float((gs * gs).sum()))
            trust = ETA * wn / (gn + DECAYS[0] * wn + EPS) if wn > 0 and gn > 0 else 1.0
            assert rows[name] == pytest.approx((wn, gn, trust), rel=1e-12)
            assert (trust == 1.0) == (name in ("a.weight", "e.weight"))  # gn == 0, wn == 0
        d = trust * (gs + DECAYS[c] * ws)
        if momentum:
            d = momentum * ms + d
            torch.testing.assert_close(m[sl], d.float(), rtol=2.0 ** -22, atol=0)  # (one fp32 ulp: both are float64)
        torch.testing.assert_close(w[sl], (ws - lr * d).float(), rtol=2.0 ** -22, atol=0)


def test_cpu_resnet_trainer_steps_under_lars():
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet import CPUResNetTrainer

    tr = CPUResNetTrainer(batch=4, seed=3, optimizer="lars", weight_decay=5e-4, norm_weight_decay=0.0, lars_eta=0.01)
    assert not tr.opt.plain and tr.opt.mapped and tr.trust_ratios() == {} and tr.v is None
    tr.load_shard(*(torch.from_numpy(a) for a in make_cifar_like(8, seed=1)))
    w0 = tr.get_flat()
    tr.step()
    ratios = tr.trust_ratios()
    assert list(ratios) == [name for name, shape, off in tr.layout() if len(shape) > 1] and len(ratios) == 21
    assert all(wn > 0 and gn > 0 and t == pytest.approx(0.01 * wn / (gn + 5e-4 * wn)) for wn, gn, t in ratios.values())
    assert int(tr.opt_step[0]) == 1 and bool(torch.isfinite(tr.params).all()) and not torch.equal(tr.params, w0)
    assert {k: tr.opt.meta()[k] for k in ("name", "lars_eta", "lars_eps")} == dict(name="lars", lars_eta=0.01, lars_eps=0.0)
    assert set(tr.state_extra()) == set(CPUResNetTrainer(batch=4, lr_warmup_steps=1).state_extra())  # no new state
    with pytest.raises(ValueError, match="lars"):
        CPUResNetTrainer(batch=4).trust_ratios()


def test_refusals_and_flags(monkeypatch):
    from serverless_learn_amd.models.mlp import CPUTrainer

    s, plain = OptSpec(optimizer="lars"), OptSpec()
    assert (s.lars, s.plain, s.grouped, s.mapped, s.adamw, s.lars_eta, s.lars_eps) == (True, False, False, True, False, 1e-3, 0.0)
    assert plain.plain and not plain.mapped and "lars_eta" not in plain.meta() and "name" not in plain.meta()
    for bad in (dict(lars_eta=0.0), dict(lars_eta=-1.0), dict(lars_eta=math.nan), dict(lars_eta=math.inf),
                dict(lars_eps=-1e-9), dict(lars_eps=math.nan), dict(lars_eps=math.inf)):
        for make in (OptSpec, lambda **kw: Config(model="resnet18", **kw)):
            with pytest.raises(ValueError, match=next(iter(bad))):
                make(optimizer="lars", **bad)
    with pytest.raises(ValueError, match="lars.*mlp"):
        CPUTrainer(batch=4, optimizer="lars")
    for model in ("mlp", "simulate"):
        with pytest.raises(ValueError, match="lars.*" + model):
            Config(model=model, optimizer="lars")
    for k, v in dict(SL_MODEL="resnet18", SL_OPTIMIZER="lars", SL_LARS_ETA="0.002", SL_LARS_EPS="1e-8").items():
        monkeypatch.setenv(k, v)
    e = Config.from_env()
    assert (e.optimizer, e.lars_eta, e.lars_eps) == ("lars", 0.002, 1e-8)
