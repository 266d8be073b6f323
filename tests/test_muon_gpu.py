"""Muon on the GPU (csrc/kernels/muon.hip) against ops/optim.py's float64 Newton-Schulz reference.

The orthogonaliser's bound is not a constant: for each case d0 is the relative Frobenius error of the bf16 emulation
(newton_schulz(emulate=True)) against the unrounded iteration, over the whole matrix and over its worst row and
column, and the kernels must stay within 2 d0 in each of the three.  They differ from the emulation only by the
order of their fp32 accumulation, which flips single bf16 roundings: a second error of at most the emulation's own
size, and the triangle inequality gives 2.  What compares bits between builds is computed by one SL_DETERMINISTIC=1
child process (this file's ``__main__``), as in tests/test_groupnorm_gpu.py."""
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from serverless_learn_amd.ops import cnn as K
from serverless_learn_amd.ops import optim as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
# one tile; tall; n no power of two; several row tiles and split-K; the tall case with the largest working side;
# three tensors in one plan
CASES = {"64x64": [(64, 64)], "128x64": [(128, 64)], "64x576": [(64, 576)], "256x1152": [(256, 1152)],
         "512x256": [(512, 256)], "grouped": [(64, 576), (128, 64), (256, 1152)], "zeros": [(64, 576)]}


def _plan(shapes):
    layout, off = [], 0
    for i, (m, n) in enumerate(shapes):
        layout.append([f"t{i}.weight", [m, n], off])
        off += m * n
    layout.append(["tail.bias", [10], off])  # a non-Muon tensor that ends the vector with a scalar tail
    return O.muon_plan(layout, off + 10)


def _orthogonalize(shapes, us, steps=5):
    """O of every tensor of a hand-made plan whose gradients are ``us`` (momentum 0: u = g), from the launches."""
    plan = _plan(shapes)
    b = O.MuonBuffers(plan, DEV)
    g = torch.zeros(plan.n)
    for (off, m, n, *_), u in zip(plan.tensors.tolist(), us):
        g[off:off + m * n] = u.reshape(-1)
    g, mom = g.to(DEV), torch.zeros(plan.n, device=DEV)
    O.muon_orthogonalize(g, mom, b, 0.0, True, steps)
    torch.cuda.synchronize()
    assert torch.equal(mom[:plan.n - 10], g[:plan.n - 10]) and not bool(mom[-10:].any())
    return [b.matrix(t, steps).float().cpu().double() for t in range(len(shapes))], b


def _errors(x, ref):
    """Relative Frobenius error over the whole matrix, the worst row and the worst column."""
    d = x - ref
    return (float(d.norm() / ref.norm()), float((d.norm(dim=1) / ref.norm(dim=1)).max()),
            float((d.norm(dim=0) / ref.norm(dim=0)).max()))


def _inputs(case):
    gen = torch.Generator().manual_seed(len(case))
    return [torch.zeros(m, n) if case == "zeros" else torch.randn(m, n, generator=gen) for m, n in CASES[case]]


@pytest.mark.parametrize("case", list(CASES))
def test_orthogonaliser_matches_float64(case):
    us = _inputs(case)
    outs, b = _orthogonalize(CASES[case], us)
    for (m, n), u, o, nrm in zip(CASES[case], us, outs, b.norms.tolist()):
        assert o.shape == (m, n) and abs(nrm - float(u.double().norm())) <= 2 * U * nrm
        if case == "zeros":
            assert not bool(o.any())  # exact zeros, no NaN
            continue
        exact = O.newton_schulz(u, 5, emulate=False)
        d0, err = _errors(O.newton_schulz(u, 5, emulate=True), exact), _errors(o, exact)
        print(case, (m, n), "kernel", err, "emulation", d0, "ratios", [e / d for e, d in zip(err, d0)])
        assert all(e <= 2 * d for e, d in zip(err, d0))


@pytest.mark.parametrize("shape", [(64, 576), (128, 64)])
def test_hadamard_input_keeps_its_structure_exactly(shape):
    """u: the 64 x 64 Sylvester Hadamard matrix, zero-padded.  Every Gram off-diagonal is an exact sum that cancels,
    so O is exactly zero where u is, and sigma u elsewhere for one scalar sigma."""
    h = torch.ones(1, 1)
    for _ in range(6):
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    u = torch.zeros(shape)
    u[:64, :64] = h
    (o,), _ = _orthogonalize([shape], [u])
    assert torch.equal(o * (u == 0), torch.zeros_like(o))
    blk = o[:64, :64] * h.double()  # sigma everywhere, if the signs are u's
    sigma, top = float(blk.mean()), float(blk.abs().max())
    print("sigma", sigma, "spread", float(blk.max() - blk.min()))
    assert sigma > 0 and float((blk - sigma).abs().max()) <= 2 * 2.0 ** (math.floor(math.log2(top)) - 7)


def _trainer(**kw):
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    tr = FusedResNetTrainer(batch=8, device=DEV, seed=2, optimizer="muon", momentum=0.9, weight_decay=5e-4, **kw)
    tr.load_shard(*(torch.from_numpy(a) for a in make_cifar_like(16, seed=5)))
    return tr


def test_engine_update_matches_the_reference():
    tr = _trainer(bias_weight_decay=1e-4)
    tr.compute_grads()
    w0, m0, g = tr.params.cpu(), tr.mom.cpu(), tr.grad.cpu()
    # every other element: what the grouped SGD launch leaves on the same inputs, bit for bit
    w2, m2, b = tr.params.clone(), tr.mom.clone(), tr.muon_buf
    O.sgd_flat_lr_groups(w2, tr.grad, m2, torch.zeros_like(tr.opt_step), None, b.cls, tr.opt.decays(), lr=tr.lr,
                         momentum=0.9)
    tr._update()
    torch.cuda.synchronize()
    plan, spec, w1, m1 = tr.muon_plan, tr.opt, tr.params.cpu(), tr.mom.cpu()
    rest = torch.from_numpy(np.repeat(plan.block_map, 64)[:plan.n] == O.LARS_NO_TENSOR)
    assert torch.equal(w1[rest], w2.cpu()[rest]) and torch.equal(m1[rest], m2.cpu()[rest]) and int(tr.opt_step[0]) == 1
    assert torch.equal(tr.shadow.cpu(), w1.bfloat16())
    rw, rm = w0.clone(), m0.clone()
    # the reference update, its Newton-Schulz part left to the loop below: the momentum is one fma
    norms = O.muon_update(rw, rm, g, spec.lr_at(0), 0.9, spec.decays(), plan, only=())
    assert torch.equal(m1[~rest], rm[~rest])
    got = tr.muon_norms()
    assert list(got) == list(plan.names) and all(abs(got[k] - v) <= 2 * U * v for k, v in zip(plan.names, norms))
    lr, worst = spec.lr_at(0), 0.0
    for name, (off, m, n, *_) in zip(plan.names, plan.tensors.tolist()):
        if name.startswith("layer4") and name not in ("layer4.1.conv2.weight", "layer4.0.down.weight"):
            continue  # (their float64 references would take this test past a few seconds)
        sl = slice(off, off + m * n)
        u = O.fma32(0.9, rm[sl], g[sl]).view(m, n)
        exact, s = O.newton_schulz(u, 5, emulate=False), math.sqrt(max(1.0, m / n))
        d0 = float((O.newton_schulz(u, 5, emulate=True) - exact).norm() / exact.norm())
        ref = w0[sl].double() * (1.0 - lr * 5e-4) - lr * s * exact.reshape(-1)
        err = float((w1[sl].double() - ref).norm())
        bound = 2 * d0 * lr * s * float(exact.norm()) + 4 * U * float(w0[sl].double().norm())
        worst = max(worst, err / bound)
        assert err <= bound, (name, err, bound)
    print("engine: worst weight error over its bound", worst)


def _digest(*tensors):
    return hashlib.sha256(b"".join(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
                                   for t in tensors)).hexdigest()


def _update_digest():
    """One update of the grouped plan from seeded state: the digest of (w, mom, shadow, O)."""
    plan = _plan(CASES["grouped"])
    b, gen = O.MuonBuffers(plan, DEV), torch.Generator().manual_seed(7)
    w, g, mom = (torch.randn(plan.n, generator=gen).mul(s).to(DEV) for s in (0.1, 0.01, 0.01))
    sh, step = torch.zeros(plan.n, dtype=torch.bfloat16, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    O.muon_orthogonalize(g, mom, b, 0.9, True, 5)
    O.sgd_flat_muon(w, g, mom, step, None, b, (5e-4, 0.0, 1e-4), lr=0.05, momentum=0.9, shadow=sh)
    torch.cuda.synchronize()
    return _digest(w, mom, sh, b.out(5))


@pytest.fixture(scope="module")
def det_child():
    env = dict(os.environ, SL_DETERMINISTIC="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=280)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["deterministic_build"], r
    return r


def test_same_bits_twice_in_both_builds_and_under_a_graph(det_child):
    first = _update_digest()
    assert _update_digest() == first and det_child["digest"] == first
    assert det_child["graph"] == {"captured": True, "changed_vs_eager": [], "opt_step": 5, "finite": True}


def test_launchers_refuse_bad_arguments_and_write_nothing():
    plan = _plan(CASES["grouped"])
    b, lib, s, p = O.MuonBuffers(plan, DEV), O.N.lib(), O.N.stream_ptr(), lambda t: t.data_ptr()
    w, g, mom = (torch.full((plan.n,), v, device=DEV) for v in (1.0, 0.5, 0.25))
    step, th, T = torch.zeros(1, dtype=torch.int32, device=DEV), b.tensors_h, b.T
    tab = [th.ctypes.data, p(b.tensors), T]
    ok = {"sl_muon_prep": [p(g), p(mom), p(b.chunks), len(plan.chunks), 0.9, 1, p(b.partials), *tab, p(b.tiles),
                           len(plan.tiles), p(b.x[0]), p(b.norms)],
          "sl_muon_gram": [p(b.x[0]), *tab, p(b.gram_tiles), len(plan.gram_tiles), p(b.ws), p(b.tri_tiles),
                           len(plan.tri_tiles), p(b.a)],
          "sl_muon_poly": [p(b.a), *tab, p(b.poly_tiles), len(plan.poly_tiles), p(b.b)],
          "sl_muon_apply": [p(b.x[0]), p(b.b), *tab, p(b.tiles), len(plan.tiles), p(b.x[1])],
          "sl_sgd_flat_muon": [p(w), p(g), p(mom), None, plan.n, p(step), None, 0, 0.1, 0.9, 5e-4, 0.0, 0.0, 1.0, 1.0,
                               p(b.cls), p(b.block_map), *tab, p(b.x[0]), p(b.x[1]), 5]}
    # tensor tables the host check refuses: a side that is no multiple of 64, a working side past 512
    odd, big = th.copy(), th.copy()
    odd[0, 2], big[2, 1:3] = 96, (576, 1152)
    bad = {"sl_muon_prep": [(0, None), (1, None), (2, None), (3, 0), (6, None), (7, None), (7, odd.ctypes.data),
                            (7, big.ctypes.data), (8, None), (10, None), (12, None), (13, None), (0, p(g) + 4)],
           "sl_muon_gram": [(0, None), (1, odd.ctypes.data), (4, None), (6, None), (7, None), (9, None)],
           "sl_muon_poly": [(0, None), (1, big.ctypes.data), (4, None), (6, None), (6, p(b.a))],
           "sl_muon_apply": [(0, None), (1, None), (2, odd.ctypes.data), (5, None), (7, None), (7, p(b.x[0]))],
           "sl_sgd_flat_muon": [(0, None), (1, None), (2, None), (4, 0), (5, None), (15, None), (16, None), (17, None),
                                (17, big.ctypes.data), (20, None), (22, 0), (22, 9), (14, 0.0)]}
    assert all(getattr(lib, fn)(*a[:i], v, *a[i + 1:], s) != 0 for fn, a in ok.items() for i, v in bad[fn])
    torch.cuda.synchronize()
    assert bool((w == 1).all()) and bool((mom == 0.25).all()) and not any(
        bool(t.any()) for t in (*b.x, b.a, b.b, b.ws, b.partials, b.norms))
    assert all(getattr(lib, fn)(*a, s) == 0 for fn, a in ok.items())
    torch.cuda.synchronize()
    assert bool(b.x[1].any()) and bool(b.norms.all()) and not bool((w == 1).all())


def _child():
    """SL_DETERMINISTIC=1: the update's digest, and two eager + three replayed steps against five eager."""
    out = {"deterministic_build": K.deterministic(), "digest": _update_digest()}
    a, b = _trainer(), _trainer()
    a.capture(warmup=2)
    for _ in range(3):
        a.step()
    for _ in range(5):
        b.step()
    torch.cuda.synchronize()
    out["graph"] = {"captured": a.graph is not None and b.graph is None, "opt_step": int(a.opt_step[0]),
                    "changed_vs_eager": [k for k in ("params", "mom", "shadow") if not
                                         torch.equal(getattr(a, k), getattr(b, k))],
                    "finite": bool(torch.isfinite(a.params).all())}
    a.drop_graphs()
    print(json.dumps(out))


if __name__ == "__main__":  # the child process of det_child
    _child()
