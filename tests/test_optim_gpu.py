"""AdamW and the device-side learning-rate schedules on the GPU (csrc/kernels/mlp_fused.hip
RULE_ADAMW / RULE_SGD_LR, elementwise.hip opt_flat_kernel): every update path against the
float64 reference rules of ops/optim.py, graph replays with the device-resident optimizer
step, exact resume, the xGMI update, and the ResNet engine.

The replay harness: an identity ``allreduce`` hook records each step's reduced fp32 gradient;
the recorded gradients are replayed through float64 ``adamw_update`` / ``sgd_update`` +
``lr_at`` from the fp32 initial parameters, which isolates the optimizer from the bf16
gradient noise.  Bounds are fp32 rounding bounds (derived, not measured):

* parameters: ``|w - w_ref| <= 1e-6`` -- N (2^-24 |w| + ~16 * 2^-24 lr |u|) with |w| <= 0.07,
  |u| <= 3.2 is ~6e-8; an off-by-one ``t`` at step 1 moves w by ~3e-4;
* ``v``: relative 4e-6 (floor 1e-30) -- ~4 N roundings of 6e-8, 8x below the 3e-5 error of an
  fp32 ``1 - beta2``;
* ``m``: ``2^-18 max_k |g_k|`` elementwise (m can cancel).
"""
import os
import subprocess
import sys

import pytest
import torch

from serverless_learn_amd.ckpt import format as ckfmt
from serverless_learn_amd.ops.optim import OptSpec, lr_at

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N_STEPS = 6
ADAMW = dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2)
COSINE = dict(lr_schedule="cosine", lr_warmup_steps=3, lr_decay_steps=8)
W_TOL, V_RTOL, V_FLOOR, M_TOL = 1e-6, 4e-6, 1e-30, 2.0 ** -18


def _shard():
    from serverless_learn_amd.data.synthetic import make_mnist_like

    x, y = make_mnist_like(256, seed=3)  # two batches of 128: the cursor walks
    return torch.from_numpy(x), torch.from_numpy(y)


def _mlp(batch=128, seed=1, **kw):
    from serverless_learn_amd.models.mlp import FusedMLPTrainer

    tr = FusedMLPTrainer(batch=batch, device=DEV, seed=seed, **kw)
    tr.load_shard(*_shard())
    return tr


def _replay(spec: OptSpec, w0: torch.Tensor, grads: list, has_mom: bool = True):
    """The recorded gradients through the float64 reference rule: (w, m, v)."""
    w = w0.double().clone()
    m = torch.zeros_like(w) if has_mom else None
    v = torch.zeros_like(w) if spec.adamw else None
    for k, g in enumerate(grads):
        spec.update(w, m, v, g.double(), k)
    return w, m, v


def _check_state(w, m, v, ref, grads, what=""):
    """The three bounds of the module docstring; prints each figure before it asserts."""
    wr, mr, vr = ref
    gmax = torch.stack([g.abs() for g in grads]).max(0).values.double()
    ew = float((w.double() - wr).abs().max())
    print(f"{what} max |w - w_ref| = {ew:.3e} (bound {W_TOL:.0e})")
    assert ew <= W_TOL, (what, ew)
    if m is not None:
        em = (m.double() - mr).abs()
        print(f"{what} max |m - m_ref| / max_k |g_k| = {float((em / gmax.clamp_min(1e-300)).max()):.3e} "
              f"(bound {M_TOL:.3e})")
        assert bool((em <= M_TOL * gmax).all()), (what, float((em - M_TOL * gmax).max()))
    if v is not None:
        ev = (v.double() - vr).abs()
        print(f"{what} max |v - v_ref| / v_ref = {float((ev / vr.clamp_min(V_FLOOR)).max()):.3e} (bound {V_RTOL:.0e})")
        assert bool((ev <= V_RTOL * vr + V_FLOOR).all()), (what, float((ev / vr.clamp_min(V_FLOOR)).max()))


def _recorded_run(batch, steps=N_STEPS, **kw):
    """A trainer stepped eagerly through the update-from-gradient path with the recording hook."""
    from serverless_learn_amd.models.mlp import N_PARAMS

    tr = _mlp(batch=batch, **kw)
    w0 = tr.get_flat().cpu()
    rec = []
    tr.allreduce = lambda g: rec.append(g[:N_PARAMS].clone())
    for _ in range(steps):
        tr.step()
    torch.cuda.synchronize()
    return tr, w0, [g.cpu() for g in rec]


def _mlp_state(tr):
    from serverless_learn_amd.models.mlp import N_PARAMS

    n = N_PARAMS
    return (tr.get_flat().cpu(), tr.mom[:n].cpu() if tr.mom is not None else None,
            tr.v[:n].cpu() if tr.v is not None else None)


def _same_trainers(a, b, what):
    """Bit-identical: parameters, both moments, every shadow and the W1 row sums."""
    for name in ("params", "mom", "v", "w1h", "w2h", "w2th", "w3h", "w3th", "r1p", "opt_step", "cursor"):
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None), (what, name)
        if ta is not None:
            assert torch.equal(ta, tb), (what, name, int((ta != tb).sum()))


@pytest.fixture(scope="module")
def adamw_update_run():
    """Test 2's batch-128 trainer after N steps: the reference run of the bit-identity tests."""
    return _recorded_run(128, **ADAMW)


# ---- 1. the flat kernels ----
@pytest.mark.parametrize("n,shadow,sched", [(1027, True, True), (1027, False, False),
                                            (2_097_152 + 1027, True, True)])
def test_adamw_flat_matches_float64(n, shadow, sched):
    """n = 1027: float4 body + a 3-element tail; 2,097,152 + 1027: more than one grid-stride
    sweep at the 2048-block cap.  Three steps with the device counter, grad_scale != 1."""
    from serverless_learn_amd.ops import cnn as K
    from serverless_learn_amd.ops import optim as O

    spec = OptSpec(**ADAMW, **(dict(lr_schedule="cosine", lr_warmup_steps=2, lr_decay_steps=5) if sched else {}))
    gen = torch.Generator().manual_seed(n)
    w0 = (torch.rand(n, generator=gen) * 2 - 1) * 0.07
    # gradient magnitudes over ten decades, so v spans twenty
    grads = [torch.randn(n, generator=gen) * torch.exp(torch.rand(n, generator=gen) * -23.0) for _ in range(3)]
    gscale = 0.37
    w, m, v = w0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sh = torch.zeros(n, dtype=torch.bfloat16, device=DEV) if shadow else None
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    tab = torch.from_numpy(spec.lr_table()).to(DEV) if sched else None
    for g in grads:
        O.adamw_flat(w, g.to(DEV), m, v, step, spec, tab, shadow=sh, grad_scale=gscale)
        K.cursor_bump(step)
    torch.cuda.synchronize()
    assert int(step.item()) == 3
    scaled = [g * gscale for g in grads]
    ref = _replay(spec, w0, [g.double() * gscale for g in grads])
    _check_state(w.cpu(), m.cpu(), v.cpu(), ref, scaled, f"adamw_flat n={n}")
    if shadow:
        assert torch.equal(sh, w.to(torch.bfloat16))


def test_sgd_flat_lr_matches_float64():
    from serverless_learn_amd.ops import cnn as K
    from serverless_learn_amd.ops import optim as O

    n = 1027
    spec = OptSpec(lr=0.05, momentum=0.9, weight_decay=1e-4, lr_schedule="linear", lr_warmup_steps=2,
                   lr_decay_steps=4, lr_min_ratio=0.1)
    gen = torch.Generator().manual_seed(5)
    w0 = (torch.rand(n, generator=gen) * 2 - 1) * 0.07
    grads = [torch.randn(n, generator=gen) * 0.1 for _ in range(6)]  # past the schedule's end
    w, m = w0.to(DEV), torch.zeros(n, device=DEV)
    sh = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    tab = torch.from_numpy(spec.lr_table()).to(DEV)
    for g in grads:
        O.sgd_flat_lr(w, g.to(DEV), m, step, tab, spec.momentum, spec.weight_decay, shadow=sh)
        K.cursor_bump(step)
    torch.cuda.synchronize()
    # (SGD's buffer also accumulates weight_decay * w: the m bound, in units of |g|, is AdamW's)
    _check_state(w.cpu(), None, None, _replay(spec, w0, grads), grads, "sgd_flat_lr")
    assert torch.equal(sh, w.to(torch.bfloat16)) and int(step.item()) == 6


# ---- 2. / 3. the MLP's AdamW: update from a gradient, and the fused slab update ----
def test_mlp_adamw_update_from_gradient(adamw_update_run):
    tr, w0, grads = adamw_update_run
    assert len(grads) == N_STEPS and int(tr.opt_step.item()) == N_STEPS and int(tr.cursor.item()) == N_STEPS
    assert int(tr.opt_ticket.item()) == 0
    _check_state(*_mlp_state(tr), _replay(tr.opt, w0, grads), grads, "mlp adamw B=128")


def test_mlp_adamw_update_from_gradient_64_row_tile():
    tr, w0, grads = _recorded_run(64, **ADAMW)
    assert int(tr.opt_step.item()) == N_STEPS and int(tr.cursor.item()) == N_STEPS
    _check_state(*_mlp_state(tr), _replay(tr.opt, w0, grads), grads, "mlp adamw B=64")


def test_mlp_adamw_fused_slab_path_is_bit_identical(adamw_update_run):
    """No hook: slab reduction + AdamW in one launch.  Both paths consume the same slab in the
    same order, as the SGD paths do."""
    tr = _mlp(**ADAMW)
    for _ in range(N_STEPS):
        tr.step()
    torch.cuda.synchronize()
    _same_trainers(tr, adamw_update_run[0], "fused slab vs update-from-gradient")
    assert int(tr.opt_ticket.item()) == 0


# ---- 4. graphs ----
def test_graph_replays_follow_the_device_step():
    """AdamW + cosine (warm-up 3, decay ends at 8): a 1-step graph replayed 5 times, and a 4-step
    graph driven for 11 steps (two replays + the 3-step remainder, past the schedule's end),
    equal eager steps bit for bit: the step number lives on the device."""
    kw = dict(**ADAMW, **COSINE)
    e = _mlp(**kw)
    snap = None
    for k in range(11):
        e.step()
        if k == 4:
            torch.cuda.synchronize()
            snap = {n: getattr(e, n).clone() for n in ("params", "mom", "v", "opt_step")}
    a = _mlp(**kw)
    a.capture(warmup=0)
    for _ in range(5):
        a.step()
    torch.cuda.synchronize()
    for n, t in snap.items():
        assert torch.equal(getattr(a, n), t), ("1-step graph", n)
    b = _mlp(**kw)
    b.capture(warmup=0, unroll=4)
    b.steps(11)
    torch.cuda.synchronize()
    _same_trainers(b, e, "4-step graph, 11 steps")
    assert int(b.opt_step.item()) == 11 and int(b.opt_ticket.item()) == 0


# ---- 5. schedules on SGD ----
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
def test_mlp_sgd_schedules(schedule):
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, lr_schedule=schedule, lr_warmup_steps=2, lr_decay_steps=5,
              lr_min_ratio=0.1)
    tr, w0, grads = _recorded_run(128, **kw)
    assert tr.v is None and int(tr.opt_step.item()) == N_STEPS
    _check_state(tr.get_flat().cpu(), None, None, _replay(tr.opt, w0, grads), grads, f"mlp sgd {schedule}")
    # the fused slab path under the same rule
    f = _mlp(**kw)
    for _ in range(N_STEPS):
        f.step()
    torch.cuda.synchronize()
    _same_trainers(f, tr, f"sgd {schedule}: fused slab vs update-from-gradient")


def test_mlp_sgd_schedule_exposes_lr_t():
    """momentum = 0, weight_decay = 0: each step's dw / g is -lr_t.  On the elements with
    |g| >= 1e-3 max |g|, |dw + lr_t g| <= 2e-6 lr_t |g| (1e-6 for the schedule value plus the
    update's product rounding) + 2^-24 |w_new|: the stored weight is itself rounded to fp32,
    half an ulp, which dw / g cannot see through (the initial weights are scaled by 2^-10 so
    that this term stays small beside the first)."""
    from serverless_learn_amd.models.mlp import N_PARAMS, init_params

    kw = dict(lr=0.05, momentum=0.0, weight_decay=0.0, lr_schedule="cosine", lr_warmup_steps=2, lr_decay_steps=5,
              lr_min_ratio=0.1)
    tr = _mlp(flat=init_params(1) * 2.0 ** -10, **kw)
    assert tr.mom is None
    rec = []
    tr.allreduce = lambda g: rec.append(g[:N_PARAMS].clone())
    ws = [tr.get_flat()]
    for _ in range(N_STEPS):
        tr.step()
        ws.append(tr.get_flat())
    torch.cuda.synchronize()
    worst, sharp = 0.0, []
    for k, g in enumerate(rec):
        g = g.double().cpu()
        w_old, w_new = ws[k].double().cpu(), ws[k + 1].double().cpu()
        lr_t = lr_at(k, 0.05, "cosine", 2, 5, 0.1)
        sel = g.abs() >= 1e-3 * g.abs().max()
        err = ((w_new - w_old) + lr_t * g).abs()[sel]
        store = (2.0 ** -24 * w_new.abs())[sel]
        bound = 2e-6 * lr_t * g.abs()[sel] + store
        worst = max(worst, float((err / (lr_t * g.abs()[sel])).max()))
        sharp.append(int((store < 1e-6 * lr_t * g.abs()[sel]).sum()))  # elements where lr_t shows to 3e-6
        assert bool((err <= bound).all()), (k, float((err - bound).max()))
    print(f"sgd cosine: max |dw + lr_t g| / (lr_t |g|) = {worst:.3e}; elements that resolve lr_t to 3e-6, "
          f"per step: {sharp}")
    assert min(sharp) > 0, sharp  # every step's lr_t is pinned by some element (the output biases at least)


# ---- 6. exact resume ----
def test_mlp_resume_is_bit_exact_with_adamw_cosine():
    from serverless_learn_amd.models.mlp import N_PARAMS

    kw = dict(**ADAMW, **COSINE)
    a = _mlp(**kw)
    for _ in range(3):
        a.step()
    extra = a.state_extra()
    assert set(extra) == {"cursor", "opt_step", "exp_avg_sq"}
    buf = ckfmt.encode(a.get_flat().cpu().numpy(), {"model": a.model_name, "step": 3}, a.mom[:N_PARAMS].cpu().numpy(),
                       extra)
    meta, params, mom, extra = ckfmt.decode_full(buf)
    for _ in range(4):
        a.step()
    b = _mlp(seed=9, **kw)
    b.opt_ticket.fill_(7)  # load_state_extra zeroes the ticket
    b.set_flat(torch.from_numpy(params))
    b.mom[:N_PARAMS].copy_(torch.from_numpy(mom))
    b.load_state_extra(extra)
    assert int(b.opt_step.item()) == 3 and int(b.opt_ticket.item()) == 0
    for _ in range(4):
        b.step()
    torch.cuda.synchronize()
    _same_trainers(a, b, "resume at 3 + 4 steps vs 7 steps")
    assert int(b.opt_step.item()) == 7
    assert any(t is b.v for t in b.buffers()) and any(t is b.opt_step for t in b.buffers())


# ---- 7. xGMI in process, W = 1 ----
@pytest.mark.parametrize("two_shot,barrier", [(False, False), (True, False), (False, True)])
def test_xgmi_update_in_process(adamw_update_run, two_shot, barrier, monkeypatch):
    """The xGMI update kernel under AdamW with a group of one: one-shot and two-shot with inline
    synchronisation, and the separate-barrier protocol; eager steps and one captured graph."""
    from serverless_learn_amd.parallel.xgmi import XgmiExchange

    if barrier:
        monkeypatch.setenv("SL_XGMI_BARRIER", "1")
    for graph in (False, True):
        tr = _mlp(**ADAMW)
        ex = XgmiExchange(tr.n_pad, 0, 1, tr.device, allgather=lambda b: [b], all_ok=lambda ok: ok, two_shot=two_shot)
        assert ex.inline_sync == (0 if barrier else 1)
        try:
            tr.enable_xgmi(ex)
            if graph:
                tr.capture(warmup=0)
            for _ in range(N_STEPS):
                tr.step()
            torch.cuda.synchronize()
            assert not ex.error()
            _same_trainers(tr, adamw_update_run[0], f"xgmi two_shot={two_shot} barrier={barrier} graph={graph}")
        finally:
            tr.drop_graphs()
            ex.close()


# ---- 8. xGMI, two ranks sharing the GPU ----
def test_xgmi_two_ranks_adamw():
    """scripts/optim_xgmi_check.py: two ranks train on different halves of one shard with AdamW
    (one-shot, then two-shot); replicas bit-identical and equal to a single-process run fed the
    rank-order sum of the recorded gradients."""
    from serverless_learn_amd.utils.gpu_share import share_gpu_env
    from serverless_learn_amd.utils.ports import reserve_port

    limit = 150
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(reserve_port()),
           os.path.join(ROOT, "scripts", "optim_xgmi_check.py"), "--same-device"]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit + 15,
                       env=share_gpu_env(dict(os.environ), 2))
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("OPTIM_XGMI_OK") == 2, p.stdout[-4000:]


# ---- 9. the ResNet engine ----
def test_resnet_adamw_matches_float64():
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    x, y = make_cifar_like(2 * 32, seed=5)
    tr = FusedResNetTrainer(batch=32, device=DEV, seed=2, lr_warmup_steps=2, **ADAMW)
    tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
    w0 = tr.get_flat().cpu()
    rec = []
    tr.allreduce = lambda g: rec.append(g.clone())
    for _ in range(3):
        tr.step()
    torch.cuda.synchronize()
    grads = [g.cpu() for g in rec]
    assert int(tr.opt_step.item()) == 3 and int(tr.cursor.item()) == 3
    # the parameter bound at the engine's lr: the same 1e-3 the bound was derived for
    _check_state(tr.get_flat().cpu(), tr.mom.cpu(), tr.v.cpu(), _replay(tr.opt, w0, grads), grads, "resnet adamw")
    assert torch.equal(tr.shadow, tr.params.to(torch.bfloat16))
    assert {"opt_step", "exp_avg_sq"} <= set(tr.state_extra())


def test_resnet_adamw_graph_equals_eager_in_deterministic_build():
    """SL_DETERMINISTIC=1 (a process loads one kernel library: a child process): 3 captured-graph
    steps equal 3 eager steps bit for bit in parameters and both moments."""
    import json

    out = subprocess.run(["timeout", "-k", "10", "200", sys.executable,
                          os.path.join(ROOT, "scripts", "optim_resnet_det.py"), "32", "3"],
                         env=dict(os.environ, SL_DETERMINISTIC="1"), capture_output=True, text=True, timeout=215)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["deterministic_build"] and r["finite"], r
    assert r["params_identical"] and r["mom_identical"] and r["v_identical"], r
    assert r["opt_step"] == [4, 4], r


# ---- 10. the default is untouched ----
def test_default_trainer_has_no_optimizer_state_or_launches():
    tr = _mlp()
    assert tr.v is None and tr.opt_step is None and tr.opt_ticket is None and tr.lr_tab is None
    assert set(tr.state_extra()) == {"cursor"} and tr.buffers() == []
    assert {l.name for l in tr._launches().values() if not isinstance(l, list)} == {
        "sl_mlp_rows", "sl_mlp_wgrad", "sl_mlp_sgd"}
    ad = _mlp(**ADAMW)
    lc = ad._launches()
    assert (lc["sgd"].name, lc["update"].name, lc["reduce"].name) == ("sl_mlp_opt", "sl_mlp_opt", "sl_mlp_sgd")
    # a new hyper-parameter rebuilds the launches, as a new lr does
    ad.set_optimizer(beta2=0.95)
    assert ad._launches() is not lc
