"""Sharpness-aware minimization on the GPU (csrc/kernels/sam.hip) against float64 (ops/optim.py sam_perturb_reference),
on test_sam.py's cases, and in the ResNet engine.  Bounds, derived and not tuned to a run: every (T g)^2 is the
reference's own fp64 value, so the norms differ by the order of two sums of n non-negative terms, n 2^-52 relative;
w' and the reference round the same real number, up to that norm error, once to fp32: one ulp.  What compares bits
between builds or between runs of a step is computed by one SL_DETERMINISTIC=1 child process (this file's __main__)."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from serverless_learn_amd.ops import optim as O
from test_sam import ETA, RHO, case, ulps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda t: t.detach().cpu().contiguous().view(torch.uint8)  # noqa: E731
same = lambda a, b: torch.equal(bits(a), bits(b))  # noqa: E731


def perturb(w, g, cls, adaptive, rho=RHO):
    """The three launches on device copies of (w, g): (buffers, w', shadow)."""
    b, dw, dg = O.SamBuffers(cls, w.numel(), DEV), w.to(DEV), g.to(DEV)
    sh = torch.zeros(w.numel(), dtype=torch.bfloat16, device=DEV)
    O.sam_norms(dw, dg, b, adaptive, ETA)
    O.sam_scale(b, rho)
    O.sam_perturb(dw, dg, sh, b, adaptive, ETA)
    torch.cuda.synchronize()
    return b, dw, sh


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("n", [64, 4096, 4096 + 64, 3 * 4096 + 320])  # one chunk, an exact one, a ragged last one
def test_kernels_match_float64(n, adaptive):
    w, g, cls = case(n)
    ref, nrm, _ = O.sam_perturb_reference(w, g, cls, RHO, adaptive, ETA)
    b, dw, sh = perturb(w, g, cls, adaptive)
    got_nrm, got_scale = b.out.tolist()
    print(f"n={n} adaptive={adaptive}: |nrm - ref| / ref = {abs(got_nrm - nrm) / nrm:.3e} (bound {n * 2.0 ** -52:.3e}), "
          f"w' within {ulps(dw, ref)} ulp")
    assert abs(got_nrm - nrm) <= n * 2.0 ** -52 * nrm and got_scale == RHO / (got_nrm + 1e-12)
    assert same(b.saved, w) and same(sh, dw.bfloat16()) and ulps(dw, ref) <= 1 and not same(dw, w)
    b2, dw2, sh2 = perturb(w, g, cls, adaptive)  # the same bits from call to call
    assert same(b2.out, b.out) and same(b2.partials, b.partials) and same(dw2, dw) and same(sh2, sh)
    O.sam_restore(dw, b)
    torch.cuda.synchronize()
    assert same(dw, w)


@pytest.mark.parametrize("poison", [0.0, math.nan])
def test_a_zero_or_non_finite_gradient_leaves_the_weights(poison):
    w, g, cls = case(4096 + 64)
    g = g * 0 if poison == 0 else g.index_fill(0, torch.tensor([4100]), poison)
    b, dw, sh = perturb(w, g, cls, True)
    nrm, scale = b.out.tolist()
    assert (nrm, scale) == (0.0, RHO / 1e-12) if poison == 0 else (math.isnan(nrm) and scale == 0.0)
    assert same(dw, w) and same(b.saved, w) and same(sh, w.bfloat16())


def test_launchers_refuse_bad_arguments_and_launch_nothing():
    w, g, cls = case(4096 + 64)
    b, dw, dg = O.SamBuffers(cls, w.numel(), DEV), w.to(DEV), g.to(DEV)
    sh, p = torch.zeros(w.numel(), dtype=torch.bfloat16, device=DEV), lambda t: t.data_ptr()
    lib, s, n = O.N.lib(), O.N.stream_ptr(), w.numel()
    norms = [p(dw), p(dg), p(b.cls), n, 1, ETA, p(b.partials), 2]
    pert = [p(dw), p(dg), p(b.saved), p(sh), n, p(b.cls), 1, ETA, p(b.out)]
    bad = lambda ok, i, v: ok[:i] + [v] + ok[i + 1:]  # noqa: E731
    for i, v in [(0, None), (1, None), (2, None), (6, None), (3, 0), (3, -64), (3, n - 4), (7, 1), (7, 3)]:
        assert lib.sl_sam_norms(*bad(norms, i, v), s) != 0
    for i, v in [(0, None), (1, None), (2, None), (3, None), (5, None), (8, None), (4, 0), (4, n + 32)]:
        assert lib.sl_sam_perturb(*bad(pert, i, v), s) != 0
    assert lib.sl_sam_scale(None, 2, RHO, p(b.out), s) != 0 and lib.sl_sam_scale(p(b.partials), 0, RHO, p(b.out), s) != 0
    torch.cuda.synchronize()
    assert same(dw, w) and not bool(b.partials.any()) and not bool(b.out.any()) and not bool(b.saved.any())


def trainer(norm, **kw):
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    tr = FusedResNetTrainer(batch=4, device=DEV, in_hw=8, seed=3, norm=norm, **kw)
    tr.load_shard(*(torch.from_numpy(a) for a in make_cifar_like(8, seed=1)))  # (read as 8 x 8 records)
    return tr


@pytest.mark.parametrize("norm", ["batch", "group"])
def test_engine_step_restores_the_weights_and_keeps_the_first_pass(norm):
    kw = dict(lr=0.0, weight_decay=0.0)
    tr, off = trainer(norm, sam_rho=RHO, sam_adaptive=True, **kw), trainer(norm, **kw)
    w0 = tr.params.clone()
    for t in (tr, off):
        t.step()
    torch.cuda.synchronize()
    assert same(tr.params, w0) and same(tr.shadow, tr.params.bfloat16()) and int(tr.cursor) == 1
    run, run_off = tr.running_stats(), off.running_stats()
    assert len(run) == (20 if norm == "batch" else 0)
    assert all(same(a, b) for k in run for a, b in zip(run[k], run_off[k])) and tr.stats() == off.stats()
    st = tr.sam_stats()
    assert st["norm"] > 0 and st["scale"] == RHO / (st["norm"] + 1e-12) and math.isfinite(st["loss_perturbed"])
    assert st["loss_perturbed"] != tr.stats().loss and not same(tr.sam_buf.saved, torch.zeros_like(w0))
    assert set(tr.state_extra()) == set(off.state_extra()) and len(tr.buffers()) == len(off.buffers())
    assert off.sam_buf is None and off.sam_cls is None and off.sam_loss is None  # nothing allocated with it off


@pytest.fixture(scope="module")
def det_child():
    env = dict(os.environ, SL_DETERMINISTIC="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=280)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["deterministic_build"], r
    return r


@pytest.mark.parametrize("norm", ["batch", "group"])
def test_second_gradient_is_the_gradient_at_w_prime_and_the_graph_replays_the_eager_step(norm, det_child):
    assert det_child[norm] == {"grad_is_at_w_prime": True, "moved": True, "captured": True, "changed_vs_eager": [],
                               "cursor": 5, "finite": True}


def _child():
    """SL_DETERMINISTIC=1, per norm: the gradient a SAM step hands the update against compute_grads() of a SAM-off
    trainer moved to w' by the same launches; then two eager + three replayed steps against five eager."""
    from serverless_learn_amd.ops import cnn as K

    out = {"deterministic_build": K.deterministic()}
    for norm in ("batch", "group"):
        tr, twin = trainer(norm, sam_rho=RHO, lr=0.0), trainer(norm)
        tr.step()
        g1 = twin.compute_grads().clone()
        b, wp = tr.sam_buf, twin.params.clone()
        O.sam_norms(wp, g1, b, False, ETA)
        O.sam_scale(b, RHO)
        O.sam_perturb(wp, g1, torch.zeros_like(twin.shadow), b, False, ETA)
        moved = not torch.equal(wp, twin.params)
        twin.set_flat(wp)
        at_wp = torch.equal(tr.grad, twin.compute_grads())
        a, e = trainer(norm, sam_rho=RHO, sam_adaptive=True), trainer(norm, sam_rho=RHO, sam_adaptive=True)
        a.capture(warmup=2)
        for _ in range(3):
            a.step()
        for _ in range(5):
            e.step()
        torch.cuda.synchronize()
        state = lambda t: dict({k: getattr(t, k) for k in ("params", "shadow", "grad", "loss", "sam_loss", "mom")},  # noqa: E731
                               sam_out=t.sam_buf.out, **{k: torch.cat(v) for k, v in t.running_stats().items()})
        changed = [k for k, v in state(a).items() if not torch.equal(v, state(e)[k])]
        out[norm] = {"grad_is_at_w_prime": at_wp, "moved": moved, "captured": a.graph is not None and e.graph is None,
                     "changed_vs_eager": changed, "cursor": int(a.cursor.item()),
                     "finite": bool(torch.isfinite(a.params).all())}
        a.drop_graphs()
    print(json.dumps(out))


if __name__ == "__main__":  # the child process of det_child
    _child()
