"""Global-norm gradient clipping on the GPU (csrc/kernels/elementwise.hip clip_sumsq_kernel /
clip_scale_kernel, ops/optim.py clip_grad_norm_flat) and in both training engines.

Bounds (fp32 rounding, derived, with a 2x margin; the observed maxima are printed and recorded
in profiles/r09_clip/README.md):

* the reported norm: ``|norm_out - total64| <= 2^-22 total64`` -- the fp64 sum is rounded to
  fp32 once (2^-24; the fp64 accumulation itself adds ~n 2^-53);
* a scaled element: within ``2^-21 |g_i|`` of ``float32(g64_i * coef64)`` -- ``total``, ``total +
  1e-6``, the divide and the product each round once (4 x 2^-24 = 2^-22);
* ``coef == 1`` (``max_norm`` above the norm, or inf): the vector is bit-identical to the input.

``max_norm`` is always an fp32-representable number, so passing it to the kernel adds no rounding.
``G`` = 1024 workgroups x 256 threads x 4 floats = 1,048,576 is what one pass of the full grid
covers: ``n = G + 6`` takes a second grid-stride iteration that ends in a 2-element tail.
"""
import math

import numpy as np
import pytest
import torch

from serverless_learn_amd.ops.optim import OptSpec, clip_grad_
from test_optim_gpu import ADAMW, _check_state, _mlp, _mlp_state, _same_trainers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 1024 * 256 * 4
N_MLP = 269_322
SGD = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
NORM_RTOL, ELEM_RTOL = 2.0 ** -22, 2.0 ** -21
N_STEPS = 4
SIZES = (1, 3, 255, 1027, N_MLP, G + 6)


def _f32(v: float) -> float:
    return float(np.float32(v))


def _data(n: int, seed: int = 0) -> torch.Tensor:
    """Normal values, 1 % of the entries scaled by 1e3."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed + n))
    g[::100] *= 1e3
    return g


def _clip(g: torch.Tensor, max_norm: float):
    """clip_grad_norm_flat on a device vector with fresh scratch: the norm tensor."""
    from serverless_learn_amd.ops import optim as O

    partials, norm = O.clip_buffers(g.numel(), g.device)
    O.clip_grad_norm_flat(g, max_norm, partials, norm)
    return norm


@pytest.fixture(scope="module")
def vectors():
    """Per size: (fp32 input on the host, its float64 copy, the float64 norm); built once."""
    out = {}
    for n in SIZES:
        g = _data(n)
        g64 = g.double()
        out[n] = (g, g64, float(torch.linalg.vector_norm(g64)))
    return out


# ---- 1. the kernel against float64 ----
@pytest.mark.parametrize("factor", [0.5, 0.3, 2.0, math.inf])  # (0.5: coef rounds to 0.5f, an exact product)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_float64(vectors, n, factor):
    from serverless_learn_amd.ops import optim as O

    assert O.clip_partials(n) == min(1024, (n + 1023) // 1024) and O.clip_partials(G + 6) == G // 1024
    g, g64, total64 = vectors[n]
    max_norm = _f32(factor * total64)
    d = g.to(DEV)
    norm = _clip(d, max_norm)
    torch.cuda.synchronize()
    got = float(norm[0])
    e_norm = abs(got - total64) / total64
    print(f"n={n} factor={factor}: |norm_out - total64| / total64 = {e_norm:.3e} (bound {NORM_RTOL:.3e})")
    assert e_norm <= NORM_RTOL
    out = d.cpu()
    if factor > 1:
        assert torch.equal(out, g)  # coef == 1: bit-identical
        return
    coef64 = min(1.0, max_norm / (total64 + 1e-6))
    ref = (g64 * coef64).float().double()
    err = (out.double() - ref).abs()
    e_el = float((err / g64.abs().clamp_min(1e-300)).max())
    print(f"n={n} factor={factor}: max |g_i' - ref_i| / |g_i| = {e_el:.3e} (bound {ELEM_RTOL:.3e})")
    assert bool((err <= ELEM_RTOL * g64.abs()).all()), e_el


def test_entry_point_refuses_bad_arguments():
    from serverless_learn_amd.ops import _native as N
    from serverless_learn_amd.ops import optim as O

    lib = N.lib()
    buf = torch.ones(64, device=DEV)
    partials, norm = O.clip_buffers(64, DEV)
    s = N.stream_ptr()
    call = lambda g, n, mx, p, npart, out: lib.sl_clip_grad_norm(g, n, mx, p, npart, out, s)  # noqa: E731
    ok = (buf.data_ptr(), 64, 1.0, partials.data_ptr(), 1, norm.data_ptr())
    assert call(*ok) == 0
    assert call(None, *ok[1:]) == -1                           # null g
    assert call(buf.data_ptr() + 4, 60, *ok[2:]) == -1         # g not 16-byte aligned
    assert call(*ok[:4], 0, ok[5]) == -1                       # too few partials
    assert call(ok[0], 0, *ok[2:]) == 0 and call(ok[0], -5, *ok[2:]) == 0  # nothing to do
    assert O.clip_partials(0) == 0
    torch.cuda.synchronize()
    assert float(norm[0]) == 8.0 and float(buf[0]) == pytest.approx(1.0 / (8.0 + 1e-6), rel=1e-6)  # one clip ran


# ---- 2. bounds ----
@pytest.mark.parametrize("lead", [0, 4])
@pytest.mark.parametrize("n", [1026, G + 6])  # n % 4 == 2; 1026: a second workgroup that holds only the tail
def test_nothing_beyond_n_is_read_or_written(n, lead):
    g = _data(n, seed=1)
    total64 = float(torch.linalg.vector_norm(g.double()))
    buf = torch.full((lead + n + 8,), 1e30)
    buf[lead:lead + n] = g
    d = buf.to(DEV)
    view = d[lead:lead + n]
    assert view.data_ptr() % 16 == 0
    norm = _clip(view, _f32(0.5 * total64))
    torch.cuda.synchronize()
    out = d.cpu()
    assert torch.equal(out[lead + n:], buf[lead + n:]) and torch.equal(out[:lead], buf[:lead])
    assert abs(float(norm[0]) - total64) <= NORM_RTOL * total64  # the 1e30 sentinels are not in the sum
    assert not torch.equal(out[lead:lead + n], g)
    assert float(torch.linalg.vector_norm(out[lead:lead + n].double())) == pytest.approx(0.5 * total64, rel=1e-5)


# ---- 3. reproducibility ----
def test_bit_reproducible_from_call_to_call(vectors):
    from serverless_learn_amd.ops import optim as O

    g, _, total64 = vectors[N_MLP]
    max_norm = _f32(0.5 * total64)
    partials, norm = O.clip_buffers(N_MLP, DEV)  # the same scratch every call: nothing to reset
    outs = []
    for k in range(3):
        d = g.to(DEV)
        if k == 2:  # an unrelated launch in between
            O.to_bf16(d, torch.empty(N_MLP, dtype=torch.bfloat16, device=DEV))
        O.clip_grad_norm_flat(d, max_norm, partials, norm)
        outs.append((d.clone(), norm.clone()))
    torch.cuda.synchronize()
    for d, nm in outs[1:]:
        assert torch.equal(d, outs[0][0]) and torch.equal(nm, outs[0][1])


# ---- 4. graph ----
def test_graph_replays_match_eager_calls():
    from serverless_learn_amd.ops import optim as O

    n = 5 * 1024 + 3
    srcs = [(_data(n, seed=s) * (1.0 + s)).to(DEV) for s in range(3)]
    max_norm = _f32(0.5 * float(torch.linalg.vector_norm(srcs[0].double())))  # every source clips
    src, g = srcs[0].clone(), torch.empty(n, device=DEV)
    partials, norm = O.clip_buffers(n, DEV)
    _clip(srcs[0].clone(), max_norm)  # the kernels' code is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.copy_(src)  # the preceding captured launch refills the vector
        O.clip_grad_norm_flat(g, max_norm, partials, norm)
    for s in srcs:
        src.copy_(s)
        graph.replay()
        e = s.clone()
        e_norm = _clip(e, max_norm)
        torch.cuda.synchronize()
        assert torch.equal(g, e) and torch.equal(norm, e_norm)
    assert float(norm[0]) > max_norm  # the last replay clipped


# ---- 5. the MLP engine ----
def _first_norm(batch: int) -> float:
    tr = _mlp(batch=batch)
    g = tr.compute_grads()
    return float(torch.linalg.vector_norm(g.double()))


def _clipped_run(batch, max_norm, steps=N_STEPS, **kw):
    """A clipping trainer stepped eagerly with the recording identity hook (the hook sees the
    gradient before the clip): (trainer, w0, [gradients], [grad_norm() per step])."""
    from serverless_learn_amd.models.mlp import N_PARAMS

    tr = _mlp(batch=batch, clip_grad_norm=max_norm, **kw)
    w0 = tr.get_flat().cpu()
    rec, norms = [], []
    tr.allreduce = lambda g: rec.append(g[:N_PARAMS].clone())
    for _ in range(steps):
        tr.step()
        norms.append(tr.grad_norm())
    torch.cuda.synchronize()
    return tr, w0, [g.cpu() for g in rec], norms


@pytest.mark.parametrize("batch", [128, 64])
@pytest.mark.parametrize("kw", [SGD, ADAMW], ids=["sgd", "adamw"])
def test_mlp_clip_matches_float64(kw, batch):
    """Each step's recorded device gradient through float64 clip_grad_ + the rule (as
    test_optim_gpu.py: only the clip and the rule are under test), every step clipping."""
    max_norm = _f32(0.25 * _first_norm(batch))
    tr, w0, grads, norms = _clipped_run(batch, max_norm, **kw)
    spec: OptSpec = tr.opt
    w = w0.double().clone()
    m = torch.zeros_like(w)
    v = torch.zeros_like(w) if spec.adamw else None
    clipped, worst = [], 0.0
    for k, g in enumerate(grads):
        g64 = g.double()
        total = clip_grad_(g64, max_norm)
        assert total > max_norm, (k, total)
        worst = max(worst, abs(norms[k] - total) / total)
        spec.update(w, m, v, g64, k)
        clipped.append(g64.float())
    print(f"mlp {spec.optimizer} B={batch}: max |grad_norm() - total64| / total64 = {worst:.3e} "
          f"(bound {NORM_RTOL:.3e}); norms {[round(t, 5) for t in norms]}, max_norm {max_norm:.5f}")
    assert worst <= NORM_RTOL
    st = _mlp_state(tr)
    # SGD's momentum also accumulates weight_decay * w: only AdamW's first moment is bounded in units of |g|
    _check_state(st[0], st[1] if spec.adamw else None, st[2], (w, m, v), clipped,
                 f"mlp clip {spec.optimizer} B={batch}")
    assert set(tr.state_extra()) == set(_mlp(batch=batch, **kw).state_extra())  # nothing new is checkpointed


@pytest.mark.parametrize("kw", [SGD, ADAMW], ids=["sgd", "adamw"])
def test_mlp_clip_graphs_equal_eager(kw):
    max_norm = _f32(0.25 * _first_norm(128))
    e = _mlp(clip_grad_norm=max_norm, **kw)
    for _ in range(N_STEPS):
        e.step()
    for unroll in (1, 2):
        a = _mlp(clip_grad_norm=max_norm, **kw)
        a.capture(warmup=0, unroll=unroll)
        a.steps(N_STEPS)
        torch.cuda.synchronize()
        _same_trainers(a, e, f"clip graph unroll={unroll} vs eager")
        assert torch.equal(a.clip_norm, e.clip_norm) and a.grad_norm() > max_norm


def test_mlp_clip_inf_is_the_unclipped_reduce_update_step():
    ident = _mlp(**SGD)
    ident.allreduce = lambda g: None  # identity hook: reduce -> update launches
    inf = _mlp(clip_grad_norm=math.inf, **SGD)
    for _ in range(N_STEPS):
        ident.step()
        inf.step()
    torch.cuda.synchronize()
    _same_trainers(inf, ident, "clip inf vs identity hook")
    assert torch.equal(inf.grad, ident.grad)
    total = float(torch.linalg.vector_norm(ident.grad[:N_MLP].double()))
    assert abs(inf.grad_norm() - total) <= NORM_RTOL * total and ident.grad_norm() is None


def test_mlp_clip_follows_the_exchange():
    one = _mlp(clip_grad_norm=math.inf, **SGD)
    one.allreduce = lambda g: None
    two = _mlp(clip_grad_norm=math.inf, **SGD)
    two.allreduce = lambda g: g.mul_(2.0)
    one.step()
    two.step()
    a, b = one.grad_norm(), two.grad_norm()
    print(f"grad_norm {a!r}, with the doubling hook {b!r}")
    assert a > 0 and abs(b - 2.0 * a) <= NORM_RTOL * 2.0 * a


def test_mlp_xgmi_refuses_clipping_and_default_launches_are_unchanged():
    tr = _mlp()
    lc = tr._launches()
    assert set(lc) == {"rows", "wgrad", "sgd", "reduce", "update"}
    assert {l.name for l in lc.values()} == {"sl_mlp_rows", "sl_mlp_wgrad", "sl_mlp_sgd"}
    assert tr.clip_norm is None and tr.clip_partials is None and tr.grad_norm() is None
    c = _mlp(clip_grad_norm=1.0)
    assert c._launches()["clip"].name == "sl_clip_grad_norm" and set(c._launches()) == set(lc) | {"clip"}
    with pytest.raises(ValueError, match="clip"):
        c.enable_xgmi(object())
    c.enable_xgmi(None)
    # set_optimizer turns it on, rebuilds the launches and drops the graph; lr stays the attribute's
    tr.lr = 0.01
    tr.capture(warmup=0)
    tr.set_optimizer(clip_grad_norm=0.5)
    assert tr.graph is None and tr.lr == 0.01 and tr.opt.clip_grad_norm == 0.5
    assert "clip" in tr._launches() and tr._launches() is not lc
    tr.step()
    assert tr.grad_norm() > 0
    tr.set_optimizer(clip_grad_norm=0.0)
    assert "clip" not in tr._launches() and tr.grad_norm() is None
    tr.drop_graphs()


# ---- 6. the ResNet-18 engine ----
def test_resnet_clip():
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    x, y = make_cifar_like(2 * 32, seed=5)
    xs, ys = torch.from_numpy(x), torch.from_numpy(y)
    # max_norm = inf: measured, and the gradient is untouched
    inf = FusedResNetTrainer(batch=32, device=DEV, seed=2, clip_grad_norm=math.inf)
    inf.load_shard(xs, ys)
    rec = []
    inf.allreduce = lambda g: rec.append(g.clone())
    inf.step()
    torch.cuda.synchronize()
    assert torch.equal(inf.grad, rec[0])
    first = float(torch.linalg.vector_norm(rec[0].double()))
    e = abs(inf.grad_norm() - first) / first
    print(f"resnet inf: |grad_norm() - total64| / total64 = {e:.3e} (bound {NORM_RTOL:.3e}); total {first:.5f}")
    assert e <= NORM_RTOL
    assert FusedResNetTrainer(batch=32, device=DEV, seed=2).grad_norm() is None
    # a quarter of the first norm: eager steps, then a captured one
    max_norm = _f32(0.25 * first)
    tr = FusedResNetTrainer(batch=32, device=DEV, seed=2, clip_grad_norm=max_norm)
    tr.load_shard(xs, ys)
    worst = 0.0
    for k in range(3):
        if k == 2:
            tr.capture(warmup=0)
        tr.step()
        torch.cuda.synchronize()
        total = tr.grad_norm()
        assert total > max_norm, (k, total)
        want = max_norm * total / (total + 1e-6)
        got = float(torch.linalg.vector_norm(tr.grad.double()))
        worst = max(worst, abs(got - want) / want)
    print(f"resnet clip: max | ||grad|| - max_norm total / (total + 1e-6) | (relative) = {worst:.3e} "
          f"(bound {2.0 ** -20:.3e})")
    assert worst <= 2.0 ** -20
    assert bool(torch.isfinite(tr.params).all()) and int(tr.cursor.item()) == 3
    tr.drop_graphs()
