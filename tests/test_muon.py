"""Muon on the CPU: the Newton-Schulz reference, the plan (ops/optim.py muon_plan), the CPU ResNet trainer against
muon_update applied by hand, the refusals and the flags."""
import math

import numpy as np
import pytest
import torch

from serverless_learn_amd.config import Config
from serverless_learn_amd.ops.optim import (DECAY_BLOCK, LARS_NO_TENSOR, MUON_CHUNK, OptSpec, muon_plan, muon_update,
                                            newton_schulz)


def test_newton_schulz_keeps_singular_values_in_the_band():
    """Five unrounded iterations take the singular values of the seeded 64 x 192 Gaussian (seed 0) into
    [0.68189, 1.13432] (float64 SVD): a property of the polynomial (3.4445, -4.7750, 2.0315), which does not
    converge to 1 but oscillates around it.  The assertion is that band widened by 5 %."""
    u = torch.randn(64, 192, generator=torch.Generator().manual_seed(0))
    for x in (newton_schulz(u, 5, emulate=False), newton_schulz(u.T, 5, emulate=False).T):  # wide, and tall
        s = torch.linalg.svdvals(x)
        print("singular values", float(s.min()), float(s.max()))
        assert 0.68189 * 0.95 <= float(s.min()) and float(s.max()) <= 1.13432 * 1.05
    assert not bool(newton_schulz(torch.zeros(64, 128), 5, emulate=True).any())  # u = 0: O = 0, no NaN


def _trainer(**kw):
    from serverless_learn_amd.models.resnet import CPUResNetTrainer

    return CPUResNetTrainer(batch=2, in_hw=8, seed=3, optimizer="muon", momentum=0.9, weight_decay=5e-4, **kw)


def test_plan_names_the_conv_weights_but_the_stem():
    tr = _trainer()
    p, n = tr.muon_plan, int(tr.params.numel())
    convs = [(name, shape, off) for name, shape, off in tr.layout() if len(shape) == 4 and name != "stem.weight"]
    assert list(p.names) == [c[0] for c in convs] and len(p.names) == 19 and int(p.tensors[:, 3].sum()) == 3
    assert "stem.weight" not in p.names and "fc.weight" not in p.names
    owner = np.repeat(p.block_map, DECAY_BLOCK)[:n]
    want = np.full(n, LARS_NO_TENSOR, dtype=np.uint16)
    for t, ((name, shape, off), row) in enumerate(zip(convs, p.tensors.tolist())):
        m, k = shape[0], math.prod(shape[1:])
        assert row[:4] == [off, m, k, int(m > k)] and row[9] == m * k // MUON_CHUNK
        assert (p.chunks[row[8]:row[8] + row[9]] == np.arange(off, off + m * k, MUON_CHUNK)).all()
        want[off:off + m * k] = t
    assert (owner == want).all()  # the block map covers exactly the Muon tensors' ranges
    # every X tile once; the Gram tiles are the lower triangles, times the split-K slices
    assert len(p.tiles) == p.x_elems // MUON_CHUNK == len(p.chunks)
    assert len(p.gram_tiles) == sum(r[7] * (min(r[1], r[2]) // 64) * (min(r[1], r[2]) // 64 + 1) // 2 for r in p.tensors.tolist())


def test_cpu_trainer_step_equals_muon_update_by_hand():
    from serverless_learn_amd.data.synthetic import make_cifar_like

    tr = _trainer(muon_lr_ratio=0.5)
    assert not tr.opt.plain and tr.opt.mapped and tr.muon_norms() == {} and tr.v is None and tr.mom is not None
    tr.load_shard(*(torch.from_numpy(a) for a in make_cifar_like(4, seed=1)))
    w, m = tr.params.clone(), tr.mom.clone()
    tr.step()
    norms = muon_update(w, m, tr.grad, tr.opt.lr_at(0), 0.9, tr.opt.decays(), tr.muon_plan, 0.5, True, 5)
    assert torch.equal(tr.params, w) and torch.equal(tr.mom, m) and int(tr.opt_step[0]) == 1
    assert tr.muon_norms() == dict(zip(tr.muon_plan.names, norms)) and all(v > 0 for v in norms)
    meta = tr.opt.meta()
    assert {k: meta[k] for k in ("name", "muon_lr_ratio", "muon_nesterov", "muon_ns_steps")} == dict(
        name="muon", muon_lr_ratio=0.5, muon_nesterov=True, muon_ns_steps=5)
    with pytest.raises(ValueError, match="muon"):
        tr.trust_ratios()


def test_refusals_and_flags(monkeypatch):
    from serverless_learn_amd.models.mlp import CPUTrainer

    s, plain = OptSpec(optimizer="muon"), OptSpec()
    assert (s.muon, s.plain, s.grouped, s.mapped, s.lars) == (True, False, False, True, False)
    assert (s.muon_lr_ratio, s.muon_nesterov, s.muon_ns_steps) == (1.0, True, 5) and "muon_ns_steps" not in plain.meta()
    for bad in (dict(muon_lr_ratio=0.0), dict(muon_lr_ratio=-1.0), dict(muon_lr_ratio=math.nan),
                dict(muon_lr_ratio=math.inf), dict(muon_nesterov=2), dict(muon_ns_steps=0), dict(muon_ns_steps=9),
                dict(muon_ns_steps=2.5)):
        for make in (OptSpec, lambda **kw: Config(model="resnet18", **kw)):
            with pytest.raises(ValueError, match=next(iter(bad))):
                make(optimizer="muon", **bad)
    with pytest.raises(ValueError, match="muon.*mlp"):
        CPUTrainer(batch=4, optimizer="muon")
    for model in ("mlp", "simulate"):
        with pytest.raises(ValueError, match="muon.*" + model):
            Config(model=model, optimizer="muon")
    with pytest.raises(ValueError, match="multiples of 64"):
        muon_plan([["a.weight", [64, 96], 0]], 64 * 96)
    with pytest.raises(ValueError, match="at most 512"):
        muon_plan([["a.weight", [576, 576], 0]], 576 * 576)
    env = dict(SL_MODEL="resnet18", SL_OPTIMIZER="muon", SL_MUON_LR_RATIO="0.2", SL_MUON_NESTEROV="0", SL_MUON_NS_STEPS="3")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = Config.from_env()
    assert (e.optimizer, e.muon_lr_ratio, e.muon_nesterov, e.muon_ns_steps) == ("muon", 0.2, False, 3)
    from serverless_learn_amd.config import add_cli_args, from_args
    import argparse

    ap = argparse.ArgumentParser()
    add_cli_args(ap)
    for k in env:
        monkeypatch.delenv(k)
    c = from_args(ap.parse_args("--model resnet18 --optimizer muon --muon-lr-ratio 0.3 --muon-nesterov false "
                                "--muon-ns-steps 4".split()))
    assert (c.optimizer, c.muon_lr_ratio, c.muon_nesterov, c.muon_ns_steps) == ("muon", 0.3, False, 4)
