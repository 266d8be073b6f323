"""Per-class weight decay (``norm_weight_decay`` / ``bias_weight_decay``) on the CPU: the class
map of both models, the reference rules against ``torch.optim`` with real parameter groups, the
two CPU trainers (grouped with equal decays is the ungrouped run, bit for bit; a grouped run is
the ungrouped runs composed per class), and the OptSpec / Config / worker wiring."""
import argparse
import math

import numpy as np
import pytest
import torch

from serverless_learn_amd.models import mlp as M
from serverless_learn_amd.models import resnet as R
from serverless_learn_amd.ops import optim as O
from serverless_learn_amd.ops.optim import CLS_BIAS, CLS_NORM, CLS_WEIGHT, DECAY_BLOCK, OptSpec

pad = lambda n: (n + DECAY_BLOCK - 1) // DECAY_BLOCK * DECAY_BLOCK  # noqa: E731


# ---- 1. the class map ----
@pytest.mark.parametrize("classes", [10, 100])
def test_resnet_class_map(classes):
    spec = R.resnet18_spec("cifar", classes)
    tr = R.CPUResNetTrainer(batch=2, classes=classes, norm_weight_decay=0.0)
    cls = tr.decay_cls.numpy()
    assert cls.dtype == np.uint8 and cls.shape == (spec.n_flat // DECAY_BLOCK,)
    want = np.zeros_like(cls)
    sizes = [0, 0, 0]
    for c in spec.convs():
        sizes[CLS_WEIGHT] += pad(c.numel)
    sizes[CLS_WEIGHT] += pad(classes * 512)
    for b in spec.bns():
        for off in (b.g_off, b.b_off):
            assert off % DECAY_BLOCK == 0
            want[off // DECAY_BLOCK:(off + pad(b.c)) // DECAY_BLOCK] = CLS_NORM
            sizes[CLS_NORM] += pad(b.c)
    want[spec.fc_b // DECAY_BLOCK:(spec.fc_b + pad(classes)) // DECAY_BLOCK] = CLS_BIAS
    sizes[CLS_BIAS] = pad(classes)
    assert np.array_equal(cls, want)
    assert O.decay_class_counts(cls, spec.n_flat) == tuple(sizes) and sum(sizes) == spec.n_flat
    assert (cls[spec.fc_w // DECAY_BLOCK] == CLS_WEIGHT and cls[spec.stem_conv.off // DECAY_BLOCK] == CLS_WEIGHT)


def test_mlp_class_map():
    tr = M.CPUTrainer(batch=64, bias_weight_decay=0.0)
    cls = tr.decay_cls.numpy()
    assert cls.shape == ((M.N_PARAMS + DECAY_BLOCK - 1) // DECAY_BLOCK,)
    counts = O.decay_class_counts(cls, M.N_PARAMS)
    assert counts == (M.N_PARAMS - 522, 0, M.HIDDEN + M.HIDDEN + M.CLASSES)
    per = np.repeat(cls, DECAY_BLOCK)[:M.N_PARAMS]
    for name, shape, off, n in M.param_layout():
        assert (per[off:off + n] == (CLS_BIAS if name.endswith(".bias") else CLS_WEIGHT)).all(), name


def test_class_map_refuses_a_tensor_off_the_block_boundary():
    with pytest.raises(AssertionError, match="boundary"):
        O.decay_class_map([["a.weight", [10], 0], ["a.bias", [10], 10]], 20)
    # padding takes the class of the tensor it follows
    cls = O.decay_class_map([["a.weight", [10], 0], ["bn.weight", [3], 64], ["a.bias", [70], 192]], 320,
                            norm=("bn.weight",))
    assert cls.tolist() == [0, 1, 1, 2, 2]
    vec = O.decay_vector(cls, 320, (0.5, 0.25, 0.0))
    assert vec.dtype == torch.float64 and vec[0] == 0.5 and vec[64] == 0.25 and vec[191] == 0.25 and vec[192] == 0.0


# ---- 2. the reference rules against torch.optim with three parameter groups ----
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 5, 3, bias=False)
        self.bn = torch.nn.BatchNorm2d(5)
        self.fc = torch.nn.Linear(5, 4)

    def forward(self, x):
        return self.fc(torch.relu(self.bn(self.conv(x))).mean(dim=(2, 3)))


def _flatten(model):
    """(layout, n, norm names, {name: (offset, numel)}) with every tensor on a block boundary."""
    layout, off, where = [], 0, {}
    for name, p in model.named_parameters():
        layout.append([name, list(p.shape), off])
        where[name] = (off, p.numel())
        off += pad(p.numel())
    return layout, off, ("bn.weight", "bn.bias"), where


@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_reference_matches_torch_param_groups(rule):
    torch.manual_seed(0)
    model = _Tiny().double()
    layout, n, norm, where = _flatten(model)
    cls = O.decay_class_map(layout, n, norm)
    spec = OptSpec(lr=0.05 if rule == "sgd" else 1e-2, momentum=0.9, weight_decay=0.3, norm_weight_decay=0.1,
                   bias_weight_decay=0.0, optimizer=rule, lr_schedule="cosine", lr_warmup_steps=1, lr_decay_steps=3)
    decay = O.decay_vector(cls, n, spec.decays())
    named = dict(model.named_parameters())
    flat = torch.zeros(n, dtype=torch.float64)
    for name, (off, k) in where.items():
        flat[off:off + k] = named[name].detach().reshape(-1)
    mom, v = torch.zeros_like(flat), torch.zeros_like(flat) if rule == "adamw" else None
    groups = [{"params": [named["conv.weight"], named["fc.weight"]], "weight_decay": 0.3},
              {"params": [named["bn.weight"], named["bn.bias"]], "weight_decay": 0.1},
              {"params": [named["fc.bias"]], "weight_decay": 0.0}]
    opt = (torch.optim.SGD(groups, lr=spec.lr, momentum=0.9) if rule == "sgd"
           else torch.optim.AdamW(groups, lr=spec.lr, betas=(0.9, 0.999), eps=1e-8))
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: spec.lr_at(s) / spec.lr)
    x = torch.randn(6, 3, 8, 8, dtype=torch.float64)
    y = torch.randint(0, 4, (6,))
    for step in range(3):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(x), y).backward()
        g = torch.zeros(n, dtype=torch.float64)
        for name, (off, k) in where.items():
            g[off:off + k] = named[name].grad.reshape(-1)
        spec.update(flat, mom, v, g, step, decay)
        opt.step()
        sched.step()
    for name, (off, k) in where.items():
        # (the bound of tests/test_optim.py's torch comparisons: assert_close's defaults, float64 here)
        torch.testing.assert_close(flat[off:off + k], named[name].detach().reshape(-1), msg=name)
    per = torch.as_tensor(cls).long().repeat_interleave(DECAY_BLOCK)
    assert bool((flat[[i for i in range(n) if not any(o <= i < o + k for o, k in where.values())]] == 0).all())
    assert set(per.tolist()) == {0, 1, 2}


# ---- 3. the CPU trainers ----
def _mlp_run(steps, **kw):
    from serverless_learn_amd.data.synthetic import make_mnist_like

    x, y = make_mnist_like(128, seed=3)
    tr = M.CPUTrainer(batch=64, seed=1, **kw)
    tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
    for _ in range(steps):
        tr.step()
    return tr


def _resnet_run(steps, **kw):
    from serverless_learn_amd.data.synthetic import make_cifar_like

    x, y = make_cifar_like(8, seed=5)
    tr = R.CPUResNetTrainer(batch=4, seed=2, **kw)
    tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
    for _ in range(steps):
        tr.step()
    return tr


def _state(tr):
    return {k: getattr(tr, k) for k in ("params", "mom", "v") if getattr(tr, k) is not None}


RULES = {"sgd": dict(lr=0.05, momentum=0.9), "adamw": dict(optimizer="adamw", lr=1e-3),
         "sgd-cosine": dict(lr=0.05, momentum=0.9, lr_schedule="cosine", lr_warmup_steps=2, lr_decay_steps=5)}


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("run", [_mlp_run, _resnet_run], ids=["mlp", "resnet"])
def test_equal_decays_are_the_ungrouped_run(run, rule):
    W = 1e-2
    a = run(3, weight_decay=W, **RULES[rule])
    b = run(3, weight_decay=W, norm_weight_decay=W, bias_weight_decay=W, **RULES[rule])
    assert b.opt.grouped and not b.opt.plain and int(b.opt_step[0]) == 3
    for k, t in _state(a).items():
        assert torch.equal(t, _state(b)[k]), (k, int((t != _state(b)[k]).sum()))
    assert not hasattr(a, "decay_cls") and not hasattr(a, "decay_vec")
    assert "norm_weight_decay" not in a.state_extra() and set(a.state_extra()) | {"opt_step"} == set(b.state_extra())


@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_mlp_grouped_step_composes_the_ungrouped_runs(rule):
    W = 0.5
    g = _mlp_run(1, weight_decay=W, bias_weight_decay=0.0, **RULES[rule])
    refs = [_mlp_run(1, weight_decay=wd, **RULES[rule]) for wd in (W, 0.0)]
    per = torch.as_tensor(g.decay_cls).long().repeat_interleave(DECAY_BLOCK)[:M.N_PARAMS]
    for k, t in _state(g).items():
        a, b = _state(refs[0])[k], _state(refs[1])[k]
        assert torch.equal(t[per == CLS_WEIGHT], a[per == CLS_WEIGHT]), k
        assert torch.equal(t[per == CLS_BIAS], b[per == CLS_BIAS]), k
    assert not torch.equal(refs[0].params[per == CLS_BIAS], refs[1].params[per == CLS_BIAS])


@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_resnet_grouped_step_composes_the_ungrouped_runs(rule):
    decays = (0.5, 0.25, 0.0)
    g = _resnet_run(1, weight_decay=decays[0], norm_weight_decay=decays[1], bias_weight_decay=decays[2], **RULES[rule])
    refs = [_resnet_run(1, weight_decay=wd, **RULES[rule]) for wd in decays]
    per = torch.as_tensor(g.decay_cls).long().repeat_interleave(DECAY_BLOCK)
    for k, t in _state(g).items():
        for c in (CLS_WEIGHT, CLS_NORM, CLS_BIAS):
            assert torch.equal(t[per == c], _state(refs[c])[k][per == c]), (k, c)
    for c in (CLS_NORM, CLS_BIAS):  # the decays show: each class differs between the ungrouped runs
        assert not torch.equal(refs[0].params[per == c], refs[c].params[per == c]), c


# ---- 4. OptSpec ----
def test_optspec_groups():
    s = OptSpec(weight_decay=0.1)
    assert not s.grouped and s.plain and s.decays() == (0.1, 0.1, 0.1)
    assert "norm_weight_decay" not in s.meta() and "bias_weight_decay" not in s.meta()
    g = OptSpec(weight_decay=0.1, bias_weight_decay=0.1)
    assert g.grouped and not g.plain and g.rule == O.RULE_SGD_LR and g.lr_table() is None
    assert g.decays() == (0.1, 0.1, 0.1) and g.meta()["bias_weight_decay"] == 0.1 and "norm_weight_decay" not in g.meta()
    n = OptSpec(optimizer="adamw", weight_decay=0.1, norm_weight_decay=0)
    assert n.grouped and n.rule == O.RULE_ADAMW and n.decays() == (0.1, 0.0, 0.1)
    assert n.meta()["norm_weight_decay"] == 0 and "bias_weight_decay" not in n.meta()
    for bad in (-1.0, -1e-9, math.nan, math.inf, -math.inf):
        for field in ("norm_weight_decay", "bias_weight_decay"):
            with pytest.raises(ValueError, match=field):
                OptSpec(**{field: bad})
    with pytest.raises(AssertionError):  # a grouped spec's reference update needs its decay vector
        g.update(torch.zeros(4), torch.zeros(4), None, torch.zeros(4), 0)
    # an MLP trainer accepts norm_weight_decay: there is nothing for it to act on
    tr = M.CPUTrainer(batch=64, norm_weight_decay=0.3, weight_decay=0.1)
    assert set(tr.decay_vec.tolist()) == {0.1}


# ---- 5. Config, flags, environment, worker ----
def test_config_refusals_and_parsing(monkeypatch):
    from serverless_learn_amd.config import Config, add_cli_args, from_args

    c = Config()
    assert c.norm_weight_decay == -1 and c.bias_weight_decay == -1 and c.decay_groups == {}
    assert Config(model="resnet18", norm_weight_decay=0.0, bias_weight_decay=1e-4).decay_groups == {
        "norm_weight_decay": 0.0, "bias_weight_decay": 1e-4}
    assert Config(bias_weight_decay=0).decay_groups == {"bias_weight_decay": 0.0}
    for bad in (-0.5, -2, math.nan, math.inf):
        for field in ("norm_weight_decay", "bias_weight_decay"):
            with pytest.raises(ValueError, match=field):
                Config(model="resnet18", **{field: bad})
    for field in ("norm_weight_decay", "bias_weight_decay"):
        with pytest.raises(ValueError, match="simulate"):
            Config(model="simulate", **{field: 0.0})
    with pytest.raises(ValueError, match="no normalisation layer"):
        Config(model="mlp", norm_weight_decay=0.0)
    monkeypatch.setenv("SL_NORM_WEIGHT_DECAY", "0")
    monkeypatch.setenv("SL_BIAS_WEIGHT_DECAY", "0.25")
    monkeypatch.setenv("SL_MODEL", "resnet18")
    e = Config.from_env()
    assert e.decay_groups == {"norm_weight_decay": 0.0, "bias_weight_decay": 0.25}
    ap = argparse.ArgumentParser()
    add_cli_args(ap)
    f = from_args(ap.parse_args(["--norm-weight-decay", "-1", "--bias-weight-decay", "0.125"]))
    assert f.decay_groups == {"bias_weight_decay": 0.125}


def test_worker_passes_the_groups_on_and_logs_them_once(monkeypatch):
    from serverless_learn_amd.runtime.local_cluster import LocalCluster, fast_config
    from serverless_learn_amd.utils.log import Logger

    events = []
    emit = Logger._emit
    monkeypatch.setattr(Logger, "_emit", lambda self, level, event, **f: (events.append((event, f)),
                                                                           emit(self, level, event, **f))[1])
    c = LocalCluster(fast_config(batch=64, shard_records=256, weight_decay=0.01, bias_weight_decay=0.0, max_steps=4))
    try:
        w = c.add_worker(sync="none")
        assert c.wait_for(lambda: w.state == "done", 60), (w.state, w.step)
        assert w.trainer.opt.grouped and w.trainer.opt.decays() == (0.01, 0.01, 0.0)
        assert [f for e, f in events if e == "decay_groups"] == [
            {"weight_decay": 0.01, "norm_decay": 0.01, "bias_decay": 0.0, "weight_elements": M.N_PARAMS - 522,
             "norm_elements": 0, "bias_elements": 522}]
    finally:
        c.stop()
