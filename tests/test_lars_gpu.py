"""LARS on the GPU (csrc/kernels/lars.hip) against float64, on test_lars.py's synthetic layout and on one tensor
of 3 chunks per CU.  Bounds, with U = 2^-24 (one fp32 rounding), derived and not tuned to a run:

* norms: squares are exact in fp64; the additions behind a sum, read off the kernels, are 16 + 1 of a lane (4 float4,
  a tail element), 6 xor shuffles and 3 waves in lars_norms_kernel, then 12 chunks of a lane (768 chunks, the longest
  walk here) and 6 shuffles in lars_trust_kernel: 44 at 2^-53 each, 64 more for torch's float64 sum, 2 for the sqrts;
  fp32 enters once, at the store.  trust: both norms' chains, five fp64 operations, one store.
* update, given the kernel's own fp32 trust t and fp32 hyper-parameters: fma(wd, w, g) and d = t (.) round once each
  (2 U |d|), m' = fma(mu, m, d) once, w' = fma(-lr, m', w) once, the reference's stored m' and w' once each:
  |m' - ref| <= U (2 |m'| + 2 |d|), |w' - ref| <= U (2 |w'| + lr (|m'| + 2 |d|)).
* the engine against OptSpec.update, whose trust and hyper-parameters are float64: t, wd, mu and lr each move by up
  to U relative, which adds U lr (|d| + t wd |w| + mu |m| + |m'|) to the bound on w'."""
import numpy as np
import pytest
import torch

from serverless_learn_amd.ops import optim as O
from test_lars import C, DECAYS, EPS, ETA, NORM, state, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
L_NORM = 1 + (17 + 6 + 3 + 12 + 6 + 64 + 2) * 2.0 ** -29
L_TRUST = 1 + (2 * (17 + 6 + 3 + 12 + 6 + 64 + 2) + 5) * 2.0 ** -29
HI = 1 + 2.0 ** -20  # the bounds' second-order terms
BIG = (("big.weight", 768 * C), ("big.bias", 10))  # 768 chunks: 3 per CU
LR_TAB = np.array([0.1, 0.2, 0.3, 0.05], dtype=np.float32)
f32 = lambda v: float(np.float32(v))  # noqa: E731
MU, WD = f32(0.9), tuple(f32(d) for d in DECAYS)


def _case(sizes, seed=0):
    layout, n = synthetic(sizes) if sizes else synthetic()
    plan = O.lars_plan(layout, n, NORM if not sizes else ())
    return plan, state(layout, n, seed), O.LarsBuffers(plan, DEV)


def _round(b, w, g, m, step, tab, sh=None):
    """The three launches and the bump, as the engine's _update issues them."""
    from serverless_learn_amd.ops import cnn as K

    O.lars_norms(w, g, b)
    O.lars_trust(b, ETA, EPS, WD[0])
    O.sgd_flat_lars(w, g, m, step, tab, b, WD, momentum=MU, shadow=sh)
    K.cursor_bump(step)


@pytest.mark.parametrize("sizes", [None, BIG], ids=["synthetic", "3-chunks-per-cu"])
@pytest.mark.parametrize("momentum", [True, False])
def test_norms_trust_and_update_match_float64(sizes, momentum):
    assert int(O.N.lib().sl_lars_chunk()) == C
    plan, (w0, g0, m0), b = _case(sizes)
    w, g, m = w0.to(DEV), g0.to(DEV), m0.to(DEV) if momentum else None
    sh = torch.zeros(plan.n, dtype=torch.bfloat16, device=DEV)
    step, tab = torch.full((1,), 2, dtype=torch.int32, device=DEV), torch.from_numpy(LR_TAB).to(DEV)
    _round(b, w, g, m, step, tab, sh)
    torch.cuda.synchronize()
    out = b.out.cpu().double()
    for t, (name, (off, numel, _, _)) in enumerate(zip(plan.names, plan.tensors.tolist())):
        wn = float(w0[off:off + numel].double().square().sum().sqrt())
        gn = float(g0[off:off + numel].double().square().sum().sqrt())
        tr = ETA * wn / (gn + WD[0] * wn + EPS) if wn > 0 and gn > 0 else 1.0
        e = [abs(float(out[t, k]) - v) / v if v else abs(float(out[t, k])) for k, v in enumerate((wn, gn, tr))]
        print(name, "wn, gn, trust err / U", [x / U for x in e])
        assert e[0] <= L_NORM * U and e[1] <= L_NORM * U and e[2] <= L_TRUST * U
        if name in ("a.weight", "e.weight"):  # a zero gradient, zero weights
            assert float(out[t, 2]) == 1.0 and 0.0 in (float(out[t, 0]), float(out[t, 1]))
    rw, rm = w0.clone(), m0.clone() if momentum else None
    O.lars_update(rw, rm, g0, float(LR_TAB[2]), MU, WD, plan, ETA, EPS, trust=out[:, 2].tolist())
    lr = float(LR_TAB[2])
    ms = rm.double() if momentum else (w0.double() - rw.double()) / lr  # the reference's m' (without momentum: d)
    m1, d = ms.abs(), (ms - MU * m0.double()).abs() if momentum else ms.abs()
    gw = w.cpu()
    if momentum:
        over_m = (m.cpu().double() - rm.double()).abs() - U * (2 * m1 + 2 * d) * HI
        print("m excess", float(over_m.max()))
        assert float(over_m.max()) <= 0
    over_w = (gw.double() - rw.double()).abs() - U * (2 * rw.double().abs() + lr * (m1 + 2 * d)) * HI
    print("w excess", float(over_w.max()), "changed", int((gw != w0).sum()), "of", plan.n)
    assert float(over_w.max()) <= 0 and int(step[0]) == 3
    assert torch.equal(sh.cpu(), gw.bfloat16())  # the shadow is the stored weight, rounded to nearest even
    # classes 1 and 2 against sgd_flat_lr_groups: bit-identical at decay 0 (class 1: both rules are m' = fma(mu, m,
    # g), w' = fma(-lr, m', w)); at a decay > 0 its float4 body rounds wd w before it adds g, where this kernel's
    # single fma does not, so class 2 is held to the bound above, which over_w has just checked
    w2, m2 = w0.to(DEV), m0.to(DEV) if momentum else None
    O.sgd_flat_lr_groups(w2, g, m2, torch.full_like(step, 2), tab, b.cls, WD, momentum=MU)
    norm = torch.from_numpy(np.repeat(plan.cls, 64)[:plan.n] == 1)
    assert torch.equal(gw[norm], w2.cpu()[norm]) and int(norm.sum()) == (0 if sizes else 128)


def test_captured_replays_equal_eager_rounds():
    plan, (w0, g0, m0), b = _case(None, seed=1)
    tab = torch.from_numpy(LR_TAB).to(DEV)
    run = []
    for captured in (False, True):
        w, g, m = w0.to(DEV), g0.to(DEV), m0.to(DEV)
        step = torch.zeros(1, dtype=torch.int32, device=DEV)
        if captured:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                _round(b, w, g, m, step, tab)
        for _ in range(3):
            graph.replay() if captured else _round(b, w, g, m, step, tab)
        torch.cuda.synchronize()
        run.append((w.cpu(), m.cpu(), b.out.cpu().clone(), int(step[0])))
    assert run[0][3] == 3 and all(torch.equal(a, e) for a, e in zip(run[1][:3], run[0][:3])) and run[1][3] == 3
    assert not torch.equal(run[0][0], w0)


def test_engine_steps_under_lars(monkeypatch):
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    tr = FusedResNetTrainer(batch=32, device=DEV, seed=2, optimizer="lars", weight_decay=5e-4, norm_weight_decay=0.0,
                            lr_schedule="cosine", lr_warmup_steps=2, lr_decay_steps=8)
    tr.load_shard(*(torch.from_numpy(a) for a in make_cifar_like(64, seed=5)))
    w0, m0 = tr.params.cpu(), tr.mom.cpu()
    tr.step()
    torch.cuda.synchronize()
    g, spec, plan = tr.grad.cpu(), tr.opt, tr.lars_plan
    rw, rm = w0.clone(), m0.clone()
    rows = spec.update(rw, rm, None, g, 0, plan=plan)
    ratios = tr.trust_ratios()
    assert list(ratios) == [n for n, s, o in tr.layout() if len(s) > 1] and len(ratios) == 21
    assert all(abs(a[2] - r[2]) <= L_TRUST * U * r[2] for a, r in zip(ratios.values(), rows))
    t = torch.tensor([r[2] for r in rows] + [1.0], dtype=torch.float64)[
        torch.from_numpy(plan.block_map.astype(np.int64)).clamp(max=21).repeat_interleave(64)[:plan.n]]
    lr, mu, m1 = spec.lr_at(0), spec.momentum, rm.double().abs()
    d = (rm.double() - mu * m0.double()).abs()
    x = d + t * O.decay_vector(plan.cls, plan.n, spec.decays()) * w0.double().abs() + mu * m0.double().abs() + m1
    over = (tr.params.cpu().double() - rw.double()).abs() - U * (2 * rw.double().abs() + lr * (m1 + 2 * d + x)) * HI
    print("engine w excess", float(over.max()), "opt_step", int(tr.opt_step[0]))
    assert float(over.max()) <= 0 and int(tr.opt_step[0]) == 1
    # a default trainer's update is still the one sl_sgd_flat call, and it allocates nothing of LARS's
    plain, calls = FusedResNetTrainer(batch=32, device=DEV, seed=2), []
    monkeypatch.setattr(O.N, "call", lambda name, *a: calls.append(name))
    plain._update()
    assert calls == ["sl_sgd_flat"] and not hasattr(plain, "lars_buf") and plain.opt_step is None


def test_launchers_refuse_bad_arguments_and_write_nothing():
    plan, (w0, g0, m0), b = _case(None)
    lib, s, p = O.N.lib(), O.N.stream_ptr(), lambda t: t.data_ptr()
    w, g, step, T = w0.to(DEV), g0.to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV), len(plan.names)
    ok = {"sl_lars_norms": [p(w), p(g), p(b.chunks), len(plan.chunks), p(b.partials)],
          "sl_lars_trust": [p(b.partials), p(b.tensors), T, ETA, EPS, WD[0], p(b.out)],
          "sl_sgd_flat_lars": [p(w), p(g), None, None, plan.n, p(step), None, 0, 0.1, MU, *WD, p(b.cls), p(b.block_map),
                                 p(b.out), T]}
    # (argument, value): null pointers, n_chunks / T / n < 1, a misaligned w, eta 0
    bad = {"sl_lars_norms": [(0, None), (1, None), (2, None), (3, 0), (4, None), (0, p(w) + 4)],
           "sl_lars_trust": [(0, None), (1, None), (2, 0), (3, 0.0), (6, None)],
           "sl_sgd_flat_lars": [(0, None), (1, None), (4, 0), (5, None), (13, None), (14, None), (15, None), (16, 0)]}
    assert all(getattr(lib, fn)(*a[:i], v, *a[i + 1:], s) != 0 for fn, a in ok.items() for i, v in bad[fn])
    torch.cuda.synchronize()
    assert torch.equal(w.cpu(), w0) and not bool(b.partials.any()) and not bool(b.out.any())
    assert all(getattr(lib, fn)(*a, s) == 0 for fn, a in ok.items())
    torch.cuda.synchronize()
    assert bool(b.out.any()) and not torch.equal(w.cpu(), w0)
