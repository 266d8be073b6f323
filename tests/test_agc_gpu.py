"""Adaptive gradient clipping on the GPU (csrc/kernels/agc.hip) against float64 (ops/optim.py agc_clip_reference), on
test_agc.py's layouts.  Bounds, derived and not tuned to a run: both norms are fp64 sums whose error, whatever the
order and with the two-pass form's extra scale and product, is far below an fp32 ulp, so a stats norm is the
reference's rounded once (held to 2^-23) and s = float32(t / gn) is the reference's or its neighbour (2^-23); the
product g s rounds once in each (2 x 2^-24): |out - ref| <= 2^-22 |ref|.  An unclipped unit is bit-identical."""
import math

import pytest
import torch

from serverless_learn_amd.ops import optim as O
from test_agc import CLIP, EPS, case, extremes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits = lambda t: t.cpu().view(torch.int32)  # noqa: E731


def check(plan, w, g0, out, stats, clip=CLIP, eps=EPS, decided=True):
    """One launch's ``out`` / ``stats`` on (w, g0) against the reference: (its rows, the units whose decision is no coin
    toss).  ``decided``: all must be, a condition on the inputs; an engine's gradient is what it is, and a unit within
    1e-6 of its threshold is then held to neither outcome."""
    ref = g0.clone()
    rows = O.agc_clip_reference(w, ref, plan, clip, eps)
    sure = ~((rows[:, 1] / (clip * torch.where(rows[:, 0] < eps, eps, rows[:, 0])) - 1).abs() < 1e-6)  # (NaN: sure)
    assert bool(sure.all()) or not decided
    stats = stats.cpu().double()
    assert torch.equal((stats[:, 2] < 1)[sure], (rows[:, 2] < 1)[sure])  # the clipped set
    clipped, tossed = torch.zeros(plan.n, dtype=torch.bool), torch.zeros(plan.n, dtype=torch.bool)
    for (off, k, _, _), s, ok in zip(plan.units.tolist(), rows[:, 2].tolist(), sure.tolist()):
        clipped[off:off + k], tossed[off:off + k] = ok and s < 1, not ok
    out, same = out.cpu(), ~clipped & ~tossed
    assert torch.equal(bits(out)[same], bits(g0)[same])  # unclipped units, and everything outside the units
    over = ((out.double() - ref.double()).abs() - 2.0 ** -22 * ref.double().abs())[clipped]
    print("clipped", int((rows[:, 2] < 1).sum()), "of", len(rows), "units; excess", float(over.max()))
    assert not bool((over > 0).any())
    for r, v in zip(rows[:, :2].T, stats[:, :2].T):  # wn, gn: the reference's, rounded to fp32 (where fp32 holds it)
        fits = torch.isfinite(r) & (r < 2.0 ** 127)
        assert bool(((v - r).abs() <= 2.0 ** -23 * r)[fits].all()) and not bool(torch.isfinite(v[~torch.isfinite(r)]).any())
    return rows, sure


def launch(plan, w, g):
    b, gw, gg = O.AgcBuffers(plan, DEV), w.to(DEV), g.to(DEV)
    O.agc_clip_flat(gw, gg, b, CLIP, EPS)
    torch.cuda.synchronize()
    return b, gw, gg


@pytest.mark.parametrize("seed", [0, 1])
def test_op_matches_float64(seed):
    plan, w, g0 = case(seed)
    b, gw, gg = launch(plan, w, g0)
    rows, _ = check(plan, w, g0, gg, b.stats)
    assert rows[1, 1] == 0 and rows[2, 0] == 0 and float(b.stats[1, 1]) == 0 and float(b.stats[2, 0]) == 0
    again, first = g0.to(DEV), b.stats.clone()
    O.agc_clip_flat(gw, again, b, CLIP, EPS)
    torch.cuda.synchronize()
    assert torch.equal(bits(again), bits(gg)) and torch.equal(bits(b.stats), bits(first)) and torch.equal(bits(gw), bits(w))


@pytest.mark.parametrize("k", [64, 4608])
def test_range_and_non_finite_units(k):
    plan, w, g0 = extremes(k)
    b, _, gg = launch(plan, w, g0)
    rows, _ = check(plan, w, g0, gg, b.stats)
    st, out = b.stats.cpu().double(), gg.cpu()
    assert rows[:, 2].lt(1).tolist() == [True, True, False, False, False] and bool(torch.isfinite(out[0:2 * k]).all())
    assert not bool(torch.isfinite(st[2:4, 1]).any()) and st[2:4, 2].tolist() == [1.0, 1.0]  # (c), (d): left alone
    assert math.isinf(float(out[2 * k + 5])) and math.isnan(float(out[3 * k + 7]))
    assert float(st[4, 1]) == 2.0 ** -140 and float(st[4, 2]) == 1.0  # (e)


def test_captured_replays_equal_eager_rounds():
    plan, w0, g0 = case(2)
    b, run, graph = O.AgcBuffers(plan, DEV), [], torch.cuda.CUDAGraph()
    for captured in (False, True):
        w, g = w0.to(DEV), (8 * g0).to(DEV)
        # the op and one update launch: the weights move, so every round clips against other norms
        one = lambda: (O.agc_clip_flat(w, g, b, CLIP, EPS), O.sgd_flat(w, g, None, 0.5))  # noqa: E731
        if captured:
            torch.cuda.synchronize()
            with torch.cuda.graph(graph):
                one()
            w.copy_(w0), g.copy_(8 * g0)
        for _ in range(3):
            graph.replay() if captured else one()
        torch.cuda.synchronize()
        run.append((bits(w), bits(g), bits(b.stats)))
    assert all(torch.equal(a, e) for a, e in zip(run[1], run[0])) and not torch.equal(run[0][0], bits(w0))


def test_engine_clips_between_wstd_bwd_and_the_global_clip(monkeypatch):
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer
    from serverless_learn_amd.ops import cnn as K

    log, agc, wstd_bwd, clip = [], O.agc_clip_flat, K.wstd_bwd, O.clip_grad_norm_flat
    monkeypatch.setattr(K, "wstd_bwd", lambda *a, **k: (log.append(("wstd_bwd",)), wstd_bwd(*a, **k)))
    monkeypatch.setattr(O, "clip_grad_norm_flat", lambda *a, **k: (log.append(("clip",)), clip(*a, **k)))
    monkeypatch.setattr(O, "agc_clip_flat", lambda w, g, b, *a: (
        log.append(["agc", w.clone(), g.clone()]), agc(w, g, b, *a), log[-1].extend((g.clone(), b.stats.clone()))))
    kw = dict(batch=32, device=DEV, seed=2, weight_std=True, clip_grad_norm=1.0)
    tr, twin = FusedResNetTrainer(agc_clip=0.02, **kw), FusedResNetTrainer(**kw)
    for t in (tr, twin):
        t.load_shard(*(torch.from_numpy(a) for a in make_cifar_like(64, seed=5)))
    tr.step()
    torch.cuda.synchronize()
    assert [e[0] for e in log] == ["wstd_bwd", "agc", "clip"] and len(tr.agc_plan.units) == 4840
    _, w, before, after, stats = log[1]
    rows, sure = check(tr.agc_plan, w.cpu(), before.cpu(), after, stats, 0.02, 1e-3, decided=False)
    want, got = O.agc_summary(tr.agc_plan, rows.numpy()), tr.agc_stats()
    assert list(got) == list(want) and sum(c for _, c, _ in got.values()) >= 1
    assert all(g[0] == r[0] and abs(g[2] - r[2]) <= 2.0 ** -23 for g, r in zip(got.values(), want.values()))
    assert not bool(sure.all()) or [g[1] for g in got.values()] == [r[1] for r in want.values()]
    del log[:]
    twin.step()
    torch.cuda.synchronize()
    assert [e[0] for e in log] == ["wstd_bwd", "clip"] and twin.agc_buf is None and twin.agc_plan is None


def test_launcher_refuses_bad_arguments_and_writes_nothing():
    plan, w0, g0 = case()
    b, w, g = O.AgcBuffers(plan, DEV), w0.to(DEV), g0.to(DEV)
    lib, s, U, p = O.N.lib(), O.N.stream_ptr(), len(plan.units), lambda t: t.data_ptr()
    ok = [p(w), p(g), plan.n, b.units_h.ctypes.data, p(b.units), U, b.work_h.ctypes.data, p(b.work), len(plan.work),
          CLIP, EPS, p(b.stats)]
    # null pointers; w == g; a unit beyond the vector; clip 0 and NaN; then one bad field of a unit: n % 4 != 0, n < 4,
    # n > 4608, an offset off a 16-byte boundary, cin_real > cin, n % cin != 0
    bad = [(i, None) for i in (0, 1, 3, 4, 6, 7, 11)] + [(1, p(w)), (2, plan.n - 704), (9, 0.0), (9, math.nan)]
    tables = [b.units_h.copy() for _ in range(6)]  # (alive until the calls are made)
    for t, (row, field, v) in zip(tables, ((3, 1, 4602), (3, 1, 0), (3, 1, 4612), (3, 0, int(b.units_h[3, 0]) + 2),
                                           (3, 3, 4609), (U - 1, 2, 5))):
        t[row, field] = v
        bad.append((3, t.ctypes.data))
    assert all(lib.sl_agc_clip(*ok[:i], v, *ok[i + 1:], s) != 0 for i, v in bad)
    torch.cuda.synchronize()
    assert torch.equal(bits(g), bits(g0)) and not bool(b.stats.any())
    assert lib.sl_agc_clip(*ok, s) == 0
    torch.cuda.synchronize()
    assert bool(b.stats.any()) and not torch.equal(bits(g), bits(g0))
