"""Sharpness-aware minimization on the CPU: ops/optim.py sam_perturb_reference against numpy, the CPU ResNet trainer's
two-pass step against the same step written out, the refusals and the flags.  test_sam_gpu.py shares the cases."""
import argparse
import copy
import math

import numpy as np
import pytest
import torch

from serverless_learn_amd.config import Config, add_cli_args, from_args
from serverless_learn_amd.ops.optim import OptSpec, decay_class_map, sam_perturb_reference, trainer_class_map

RHO, ETA = 0.05, 0.01


def case(n, seed=0):
    """(w, g, cls) of n elements, seeded fp32; the blocks' classes run 0, 1, 2, 0, ..."""
    gen = torch.Generator().manual_seed(seed + n)
    return (torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 1e-2,
            (np.arange(n // 64) % 3).astype(np.uint8))


def ulps(a: torch.Tensor, b: torch.Tensor) -> int:
    """The largest distance of two fp32 vectors of one sign pattern, in units of the last place."""
    return int((a.cpu().view(torch.int32).long() - b.cpu().view(torch.int32).long()).abs().max())


@pytest.mark.parametrize("adaptive", [False, True])
def test_reference_matches_numpy(adaptive):
    layout = [["c.weight", [70, 64], 0], ["n.weight", [64], 4480], ["n.bias", [64], 4544], ["fc.bias", [10], 4608]]
    cls = decay_class_map(layout, 4672, ("n.weight", "n.bias"))
    assert sorted(set(cls.tolist())) == [0, 1, 2]
    w, g, _ = case(4672)
    g[4618:] = 0  # alignment padding
    wp, nrm, scale = sam_perturb_reference(w, g, cls, RHO, adaptive, ETA)
    w64, g64, per = w.numpy().astype(np.float64), g.numpy().astype(np.float64), np.repeat(cls, 64)
    T = np.where((per == 0) & adaptive, np.abs(w64) + ETA, 1.0)
    want_nrm = math.sqrt(float(((T * g64) ** 2)[:4096].sum()) + float(((T * g64) ** 2)[4096:].sum()))
    assert abs(nrm - want_nrm) <= 4672 * 2.0 ** -52 * want_nrm and scale == RHO / (nrm + 1e-12)
    want = torch.from_numpy((w64 + scale * T * T * g64).astype(np.float32))
    assert torch.equal(wp, want) and torch.equal(wp[4618:], w[4618:]) and not torch.equal(wp, w)
    assert adaptive or abs(float((wp.double() - w.double()).norm()) - RHO) < 1e-6  # a step of length rho
    g[7] = math.nan
    wp, nrm, scale = sam_perturb_reference(w, g, cls, RHO, adaptive, ETA)
    assert math.isnan(nrm) and scale == 0.0 and torch.equal(wp, w)


@pytest.mark.parametrize("rho, adaptive", [(0.0, False), (RHO, False), (RHO, True)])
def test_cpu_resnet_step_is_the_two_pass_step_written_out(rho, adaptive):
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet import CPUResNetTrainer, ref_grads

    tr, twin = (CPUResNetTrainer(batch=4, in_hw=8, seed=3, **kw) for kw in (dict(sam_rho=rho, sam_adaptive=adaptive), {}))
    for t in (tr, twin):
        t.load_shard(*(torch.from_numpy(a) for a in make_cifar_like(8, seed=1)))  # (read as 8 x 8 records)
    tr.step()
    xs, ys, w, run = twin.x[:4], twin.y[:4], twin.params.clone(), copy.deepcopy(twin.running)
    loss, correct, g = ref_grads(twin.spec, w, xs, ys, 0.25, run)
    if rho > 0:
        wp, nrm, scale = sam_perturb_reference(w, g, trainer_class_map(twin), rho, adaptive, ETA)
        loss2, correct2, g = ref_grads(twin.spec, wp, xs, ys, 0.25, None)
        assert not torch.equal(wp, w) and tr.sam_stats() == {
            "norm": nrm, "scale": scale, "loss_perturbed": float(loss2) / 4, "correct_perturbed": float(correct2) / 4}
    twin._opt_update(g)
    assert torch.equal(tr.params, twin.params) and torch.equal(tr.mom, twin.mom) and tr.cursor == 1
    assert all(torch.equal(a, b) for k in run for a, b in zip(tr.running[k], run[k]))
    assert (tr.stats().loss, tr.stats().accuracy) == (float(loss) / 4, float(correct) / 4)
    assert set(tr.state_extra()) == set(twin.state_extra()) and len(tr.buffers()) == len(twin.buffers())
    assert (tr.sam_cls is None) == (rho == 0) and tr.opt.plain and twin.sam_cls is None


def test_refusals_and_flags(monkeypatch):
    from serverless_learn_amd.models.mlp import CPUTrainer
    from serverless_learn_amd.models.resnet import CPUResNetTrainer

    s, off = OptSpec(sam_rho=RHO, sam_adaptive=True), OptSpec()
    assert (s.sams, s.plain, s.mapped, s.rule, s.sam_eta) == (True, True, False, off.rule, ETA) and not off.sams
    assert {k: v for k, v in s.meta().items() if k not in off.meta()} == dict(sam_rho=RHO, sam_adaptive=True, sam_eta=ETA)
    assert not [k for k in off.meta() if k.startswith("sam")]
    for bad in (dict(sam_rho=-0.1), dict(sam_rho=math.nan), dict(sam_rho=math.inf), dict(sam_eta=0.0),
                dict(sam_eta=-1e-3), dict(sam_eta=math.nan), dict(sam_eta=math.inf), dict(sam_adaptive=1)):
        for make in (OptSpec, lambda **kw: Config(model="resnet18", **kw)):
            with pytest.raises(ValueError, match=next(iter(bad))):
                make(**bad)
    with pytest.raises(ValueError, match="sam_rho.*mlp"):
        CPUTrainer(batch=4, sam_rho=RHO)
    with pytest.raises(ValueError, match="sam_rho.*accum"):
        CPUResNetTrainer(batch=4, in_hw=8, sam_rho=RHO, accum_steps=2)
    tr = CPUResNetTrainer(batch=4, in_hw=8, sam_rho=RHO)
    with pytest.raises(ValueError, match="sam_rho.*accum"):
        tr.set_accum(2)
    tr.set_accum(1)
    with pytest.raises(ValueError, match="sam"):
        CPUResNetTrainer(batch=4, in_hw=8).sam_stats()
    for kw in (dict(model="mlp"), dict(model="simulate"), dict(model="resnet18", accum_steps=2),
               dict(model="resnet18", global_batch=4096)):
        with pytest.raises(ValueError, match="sam_rho"):
            Config(sam_rho=RHO, **kw)
    for k, v in dict(SL_MODEL="resnet18", SL_SAM_RHO="0.1", SL_SAM_ADAPTIVE="1", SL_SAM_ETA="0.02").items():
        monkeypatch.setenv(k, v)
    c = Config.from_env()
    assert (c.sam_rho, c.sam_adaptive, c.sam_eta) == (0.1, True, 0.02)
    ap = argparse.ArgumentParser()
    add_cli_args(ap)
    c = from_args(ap.parse_args(["--sam-rho", "2.0", "--sam-adaptive", "false", "--sam-eta", "0.5"]))
    assert (c.sam_rho, c.sam_adaptive, c.sam_eta) == (2.0, False, 0.5)
