"""Adaptive gradient clipping on the CPU: ops/optim.py agc_clip_reference against timm's few lines, its two-pass norms at
the ends of the fp32 range, the CPU ResNet trainer, the refusals and the flags.  test_agc_gpu.py shares the cases."""
import math

import pytest
import torch

from serverless_learn_amd.config import Config
from serverless_learn_amd.models.resnet import ConvSpec
from serverless_learn_amd.ops.optim import OptSpec, agc_clip_reference, agc_plan

CLIP, EPS = 0.05, 1e-3
# (name, rows, k, cin, cin_real): every round count of the kernel (1, 3, 5, 9, 18), two padded stems (n = 72, 392) and
# banks of 1, 5 and 8 rows; then the 1-D units
BANKS = (("s3", 5, 3, 8, 3), ("s7", 1, 7, 8, 3), ("p4", 8, 1, 4, 4), ("p64", 5, 1, 64, 64), ("c64", 8, 3, 64, 64),
         ("c128", 5, 3, 128, 128), ("c256", 1, 3, 256, 256), ("c512", 5, 3, 512, 512))
NORMS = (("n64.weight", 64), ("n64.bias", 64), ("n512.weight", 512))
RATIOS = (0.25, 0.5, 2.0, 8.0)  # gn / t of the units, in turn: no decision is a coin toss


def synthetic(banks=BANKS, norms=NORMS):
    """(layout, plan): the banks, the 1-D tensors, then an unclipped fc.weight, each on a 64-element boundary."""
    layout, convs, off = [], [], 0
    for name, shape, c in ([(b[0] + ".weight", [b[1], b[2], b[2], b[3]], b) for b in banks]
                           + [(name, [k], None) for name, k in norms] + [("fc.weight", [10, 64], None)]):
        layout.append([name, shape, off])
        convs += [ConvSpec(c[0], c[3], c[4], c[1], c[2], 1, 0, off)] if c else []
        off += (math.prod(shape) + 63) // 64 * 64
    return layout, agc_plan(layout, off, convs, [name for name, _ in norms])


def case(seed=0):
    """(plan, w, g), seeded fp32: unit i's gradient is rescaled to gn = RATIOS[i % 4] t over its real columns, with junk
    50 times larger in its padding columns; unit 1 has an all-zero g and unit 2 all-zero weights (t = clip eps)."""
    plan, gen = synthetic()[1], torch.Generator().manual_seed(seed)
    w, g = torch.randn(plan.n, generator=gen) * 0.1, torch.randn(plan.n, generator=gen)
    for i, (off, k, cin, cin_real) in enumerate(plan.units.tolist()):
        real = torch.arange(k) % cin < cin_real
        w[off:off + k] *= i != 2
        row = g[off:off + k].double()
        row *= RATIOS[i % 4] * CLIP * max(float(w[off:off + k][real].double().norm()), EPS) / float(row[real].norm())
        row[~real] *= 50.0
        g[off:off + k] = row.float() * (i != 1)
    return plan, w, g


def extremes(k):
    """(plan, w, g): five units of k elements, each named by what it pins."""
    plan = synthetic((("a", 5, 1, k, k),), ())[1]
    sign = torch.where(torch.arange(k) % 3 == 0, -1.0, 1.0)
    w, g = torch.full((plan.n,), 0.01), torch.full((plan.n,), 1e-3)
    g[0:k] = sign * 2.0 ** 63                        # (a) squares that overflow fp32
    w[k:2 * k] = sign * 2.0 ** -75                   # (b) wn far below agc_eps, and not 0
    g[2 * k + 5], g[3 * k + 7] = math.inf, math.nan  # (c), (d)
    g[4 * k:5 * k], g[4 * k + 9] = 0.0, 2.0 ** -140  # (e) one subnormal, zeros around it
    return plan, w, g


def test_reference_matches_timm():
    (layout, _), (plan, w, g0) = synthetic(), case()
    assert len(plan.units) == 38 + 3 and list(plan.units[:, 1]) == sorted(plan.units[:, 1], reverse=True)
    assert plan.work[-1].tolist() == [40, 1] and len(plan.names) == 11 and "fc.weight" not in plan.names
    g = g0.clone()
    rows = agc_clip_reference(w, g, plan, CLIP, EPS)
    assert float((rows[:, 1] / (CLIP * rows[:, 0].clamp(min=EPS)) - 1).abs().min()) > 1e-6
    hit = torch.zeros(plan.n, dtype=torch.bool)
    for (name, shape, off), cr in zip(layout[:-1], [b[4] for b in BANKS] + [0] * 3):  # timm's adaptive_clip_grad, float64
        sl = slice(off, off + math.prod(shape))
        p, q = (t[sl].double().view(shape[0] if cr else 1, -1) for t in (w, g0))
        pr, qr = (t.view(t.shape[0], -1, shape[-1])[..., :cr].reshape(t.shape[0], -1) if cr else t for t in (p, q))
        max_norm, gn = pr.norm(dim=1, keepdim=True).clamp(min=EPS) * CLIP, qr.norm(dim=1, keepdim=True)
        want = torch.where(gn > max_norm, q * (max_norm / gn.clamp(min=1e-6)), q).float().view(-1)
        torch.testing.assert_close(g[sl], want, rtol=2.0 ** -23, atol=0)
        hit[sl] = (gn > max_norm).expand_as(q).reshape(-1)
    assert torch.equal(g != g0, hit & (g0 != 0)) and 0 < int(hit.sum()) < plan.n  # the clipped set; nothing else is written
    assert int((rows[:, 2] < 1).sum()) == sum(RATIOS[i % 4] > 1 and i != 1 for i in range(41))


@pytest.mark.parametrize("k", [64, 4608])
def test_norms_at_the_ends_of_the_range_and_non_finite_units(k):
    plan, w, g0 = extremes(k)
    g, f32 = g0.clone(), lambda v: float(torch.tensor(v, dtype=torch.float64).float())
    rows = agc_clip_reference(w, g, plan, CLIP, EPS)
    assert rows[0, 1] == math.sqrt(k) * 2.0 ** 63 and rows[0, 2] < 1 and bool(torch.isfinite(g[0:k]).all())
    assert torch.equal(g[0:k], (g0[0:k].double() * f32(CLIP * float(rows[0, 0]) / float(rows[0, 1]))).float())
    assert rows[1, 0] == math.sqrt(k) * 2.0 ** -75 and rows[1, 2] < 1 and rows[1, 2] == f32(CLIP * EPS / float(rows[1, 1]))
    assert not bool(torch.isfinite(rows[2:4, 1]).any()) and rows[2:4, 2].tolist() == [1.0, 1.0]
    assert torch.equal(g[2 * k:4 * k].view(torch.int32), g0[2 * k:4 * k].view(torch.int32))  # the Inf and the NaN too
    assert rows[4, 1] == 2.0 ** -140 and rows[4, 2] == 1.0 and torch.equal(g[4 * k:], g0[4 * k:])


def test_cpu_resnet_trainer_steps_under_agc():
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet import CPUResNetTrainer

    tr, twin = (CPUResNetTrainer(batch=4, in_hw=8, seed=3, agc_clip=c) for c in (0.02, 0.0))
    for t in (tr, twin):
        t.load_shard(*(torch.from_numpy(a) for a in make_cifar_like(8, seed=1)))  # (read as 8 x 8 records)
        t.step()
    stats = tr.agc_stats()
    assert list(stats) == [n for n, s, o in tr.layout() if not n.startswith("fc.")] and len(tr.agc_plan.units) == 4840
    assert sum(u for u, c, s in stats.values()) == 4840 and sum(c for u, c, s in stats.values()) >= 1
    assert not torch.equal(tr.params, twin.params) and bool(torch.isfinite(tr.params).all())
    assert set(tr.state_extra()) == set(twin.state_extra()) and twin.agc_plan is None  # no new state
    assert tr.opt.plain and tr.opt.rule == twin.opt.rule and len(tr.buffers()) == len(twin.buffers())
    with pytest.raises(ValueError, match="agc"):
        twin.agc_stats()


def test_refusals_and_flags(monkeypatch):
    from serverless_learn_amd.models.mlp import CPUTrainer

    s, off = OptSpec(agc_clip=0.02), OptSpec()
    assert (s.agcs, s.plain, s.mapped, s.agc_eps) == (True, True, False, 1e-3) and not off.agcs
    assert {k: v for k, v in s.meta().items() if k not in off.meta()} == dict(agc_clip=0.02, agc_eps=1e-3)
    for bad in (dict(agc_clip=-0.1), dict(agc_clip=math.nan), dict(agc_clip=math.inf), dict(agc_eps=0.0),
                dict(agc_eps=-1e-3), dict(agc_eps=math.nan), dict(agc_eps=math.inf)):
        for make in (OptSpec, lambda **kw: Config(model="resnet18", **kw)):
            with pytest.raises(ValueError, match=next(iter(bad))):
                make(**bad)
    with pytest.raises(ValueError, match="agc.*mlp"):
        CPUTrainer(batch=4, agc_clip=0.02)
    for model in ("mlp", "simulate"):
        with pytest.raises(ValueError, match="agc.*" + model):
            Config(model=model, agc_clip=0.02)
    for k, v in dict(SL_MODEL="resnet18", SL_AGC_CLIP="0.04", SL_AGC_EPS="1e-4").items():
        monkeypatch.setenv(k, v)
    assert (Config.from_env().agc_clip, Config.from_env().agc_eps) == (0.04, 1e-4)
