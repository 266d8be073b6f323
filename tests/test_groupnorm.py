"""norm="group" on the CPU: the reference trainer, the refusals, the two Config flags, and exact
gradient accumulation (what GroupNorm allows and BatchNorm cannot)."""
import argparse

import pytest
import torch

from serverless_learn_amd.config import Config, add_cli_args, from_args
from serverless_learn_amd.data.synthetic import make_cifar_like
from serverless_learn_amd.models import resnet as R

HW = 16


def _shard(n, seed=3):
    x, y = make_cifar_like(n, seed=seed, hw=HW)
    return torch.from_numpy(x), torch.from_numpy(y)


def test_cpu_trainer_steps_without_running_statistics():
    x, y = _shard(4)
    tr = R.CPUResNetTrainer(batch=4, in_hw=HW, norm="group", norm_groups=8, lr=0.0, momentum=0.0, weight_decay=0.0)
    tr.load_shard(x, y)
    tr.step()
    assert tr.running_stats() == {} and tr._model_extra() == {} and tr.model_name == "resnet18-cifar-gn8"
    assert tr.norm_tensors()[:2] == ("stem_bn.weight", "stem_bn.bias")
    st, ev = tr.stats(), tr.evaluate(x, y)  # lr = 0: the same weights, and no eval mode to differ by
    assert ev.loss == pytest.approx(st.loss, rel=1e-6) and ev.accuracy == st.accuracy
    assert R.CPUResNetTrainer(batch=4).model_name == "resnet18-cifar"


def test_flags_and_refusals(monkeypatch):
    for kw in (dict(stem="imagenet"), dict(in_hw=64), dict(norm_groups=4), dict(norm_groups=128),
               dict(norm_groups=True), dict(norm="layer")):
        with pytest.raises(ValueError):
            R.CPUResNetTrainer(batch=4, **{"norm": "group", **kw})
    ap = argparse.ArgumentParser()
    add_cli_args(ap)
    cfg = from_args(ap.parse_args(["--model", "resnet18", "--norm", "group", "--norm-groups", "16"]))
    assert (cfg.norm, cfg.norm_groups) == ("group", 16)
    monkeypatch.setenv("SL_MODEL", "resnet18")
    monkeypatch.setenv("SL_NORM", "group")
    monkeypatch.setenv("SL_NORM_GROUPS", "8")
    cfg = Config.from_env()
    assert (cfg.norm, cfg.norm_groups) == ("group", 8)
    assert (Config().norm, Config().norm_groups) == ("batch", 32)
    for bad in (dict(model="mlp"), dict(model="simulate"), dict(model="resnet18", norm_groups=12),
                dict(model="resnet18", norm="instance")):
        with pytest.raises(ValueError):
            Config(**{"norm": "group", **bad})


def test_accumulated_step_equals_the_double_batch():
    """Without cross-sample coupling both gradients are the same sum of 2B per-sample gradients, each over at
    most HW * HW positions, in another order: at most A = 2B * HW * HW additions per element, so they differ by
    at most A * 2^-24 times what is added, per tensor the largest sum over the samples of |per-sample gradient|."""
    B = 2
    x, y = _shard(2 * B)
    kw = dict(in_hw=HW, norm="group", norm_groups=8, seed=5, momentum=0.0, weight_decay=0.0)
    a = R.CPUResNetTrainer(batch=B, accum_steps=2, **kw)
    b = R.CPUResNetTrainer(batch=2 * B, **kw)
    for tr in (a, b):
        tr.load_shard(x, y)
        tr.step()
    gnk = dict(norm="group", groups=8)
    w0 = R.init_params(b.spec, 5)
    mag = sum(R.ref_grads(b.spec, w0, x[i:i + 1], y[i:i + 1], 1.0 / (2 * B), None, **gnk)[2].abs()
              for i in range(2 * B))
    A = 2 * B * HW * HW
    for name, shape, off in a.layout():
        n = int(torch.tensor(shape).prod())
        d = (a.grad[off:off + n] - b.grad[off:off + n]).abs().max()
        assert float(d) <= A * 2.0 ** -24 * float(mag[off:off + n].max()), (name, float(d))
    assert a.stats().loss == pytest.approx(b.stats().loss, rel=1e-6)
