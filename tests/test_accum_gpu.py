"""Gradient accumulation on the GPU: the accumulate kernel (csrc/kernels/elementwise.hip
accum_flat_kernel, ops/optim.py accum_flat) and ``accum_steps`` in both training engines.

The definition (README, "Gradient accumulation"; the CPU trainers in test_accum.py): a step of
``accum_steps = K`` at batch cursor ``t`` runs micro-batches at cursors ``t .. t + K - 1`` with
``grad_scale = 1 / (batch * world * K)`` and applies ``((g_0 + g_1) + g_2) + ...``, summed in fp32 in that
order, through one exchange, one clip and one update.  Everything here is an equality of bits: a single
fp32 add is correctly rounded, so torch's fp32 sum of the same micro-gradients is the reference.  The
micro-gradients come from a twin trainer with the same weights, ``accum_steps = 1`` and ``world_size = K``
(the same gradient scale) through ``compute_grads()``.  The MLP's gradient is bit-reproducible from call
to call in the default build (its split-K slab is reduced in a fixed order), so the MLP cases run in
this process; the ResNet engine's is only in the deterministic build, so its cases run in one
``SL_DETERMINISTIC=1`` child (scripts/accum_resnet_det.py), as tests/test_resume_gpu.py does.
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from serverless_learn_amd.ckpt import format as ckfmt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
G = 1024 * 256 * 4
SIZES = (1, 3, 255, 1027, 269_322, G + 6)
OFFSETS = ((0, 0), (1, 1), (3, 3), (0, 2), (2, 0))  # (dst, src) view starts, in elements of 16-byte-aligned buffers
PAD = 8
SGD = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
ADAMW_COS_CLIP = dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2, lr_schedule="cosine", lr_warmup_steps=3,
                      lr_decay_steps=8)


def _data(n: int, seed: int = 0) -> torch.Tensor:
    """Normal values, 1 % of the entries scaled by 1e3 (as test_clip_gpu._data)."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed + n))
    g[::100] *= 1e3
    return g


# ---- 1. the kernel ----
@pytest.fixture(scope="module")
def vectors():
    """Per size: (dst, src) contents on the host; built once."""
    return {n: (_data(n), _data(n, seed=1)) for n in SIZES}


@pytest.mark.parametrize("add", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_is_exact(vectors, n, add):
    from serverless_learn_amd.ops import optim as O

    d0, s0 = vectors[n]
    want = (d0 + s0) if add else s0
    for od, os_ in OFFSETS:
        dbuf = torch.full((n + 2 * PAD,), 7e30)
        sbuf = torch.full((n + 2 * PAD,), -3e30)
        dbuf[od:od + n] = d0
        sbuf[os_:os_ + n] = s0
        dd, sd = dbuf.to(DEV), sbuf.to(DEV)
        assert dd.data_ptr() % 16 == 0 and sd.data_ptr() % 16 == 0
        O.accum_flat(dd[od:od + n], sd[os_:os_ + n], add)
        torch.cuda.synchronize()
        out = dd.cpu()
        assert torch.equal(out[od:od + n], want), (n, add, od, os_, int((out[od:od + n] != want).sum()))
        assert torch.equal(out[:od], dbuf[:od]) and torch.equal(out[od + n:], dbuf[od + n:]), (n, add, od, os_)
        assert torch.equal(sd.cpu(), sbuf)  # the source is only read


def test_entry_point_refuses_bad_arguments():
    from serverless_learn_amd.ops import _native as N
    from serverless_learn_amd.ops import optim as O

    lib = N.lib()
    d, s = torch.ones(64, device=DEV), torch.full((64,), 2.0, device=DEV)
    st = N.stream_ptr()
    assert lib.sl_accum_flat(d.data_ptr(), s.data_ptr(), 64, 1, st) == 0
    assert lib.sl_accum_flat(None, s.data_ptr(), 64, 1, st) == -1
    assert lib.sl_accum_flat(d.data_ptr(), None, 64, 0, st) == -1
    assert lib.sl_accum_flat(d.data_ptr() + 2, s.data_ptr(), 60, 0, st) == -1  # not 4-byte aligned
    assert lib.sl_accum_flat(d.data_ptr(), s.data_ptr(), 0, 0, st) == 0
    assert lib.sl_accum_flat(d.data_ptr(), s.data_ptr(), -5, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(d, torch.full((64,), 3.0, device=DEV)) and float(s.sum()) == 128.0  # one add ran
    with pytest.raises(AssertionError, match="overlap"):
        O.accum_flat(d[:40], d[24:], True)


def test_graph_replays_the_kernel():
    from serverless_learn_amd.ops import optim as O

    n = 5 * 1024 + 3
    acc, src = torch.zeros(n + 1, device=DEV)[1:], _data(n).to(DEV)
    O.accum_flat(acc, src, False)  # the kernel's code is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        O.accum_flat(acc, src, True)
    want = src.clone()
    for _ in range(3):
        graph.replay()
        want = want + src
    torch.cuda.synchronize()
    assert torch.equal(acc, want)


# ---- 2. the MLP engine against the twin ----
def _mnist(batches: int, batch: int):
    from serverless_learn_amd.data.synthetic import make_mnist_like

    x, y = make_mnist_like(batches * batch, seed=3)
    return torch.from_numpy(x), torch.from_numpy(y)


def _mlp(batch=256, seed=1, shard=None, **kw):
    from serverless_learn_amd.models.mlp import FusedMLPTrainer

    tr = FusedMLPTrainer(batch=batch, device=DEV, seed=seed, **kw)
    tr.load_shard(*(shard or _mnist(4, batch)))
    return tr


def _same_trainers(a, b, what):
    """Bit-identical: parameters, both moments, every shadow, the W1 row sums and both counters."""
    for name in ("params", "mom", "v", "w1h", "w2h", "w2th", "w3h", "w3th", "r1p", "opt_step", "cursor"):
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None), (what, name)
        if ta is not None:
            assert torch.equal(ta, tb), (what, name, int((ta != tb).sum()))


@pytest.mark.parametrize("kw", [SGD, ADAMW_COS_CLIP], ids=["sgd", "adamw-cosine-clip"])
def test_mlp_step_is_the_ordered_sum_of_the_twins_micro_gradients(kw):
    from serverless_learn_amd.models.mlp import N_PARAMS

    K, B, t0 = 3, 256, 2  # cursors 2, 3 and (wrapping the 4-batch shard) 0
    shard = _mnist(4, B)
    # clipping at inf: the norm is measured and the gradient left unscaled, so it can be read back
    clip = dict(clip_grad_norm=math.inf) if "optimizer" in kw else {}
    acc = _mlp(B, shard=shard, accum_steps=K, **kw, **clip)
    twin = _mlp(B, shard=shard, world_size=K, **kw, **clip)
    assert acc.grad_scale == twin.grad_scale == 1.0 / (K * B) and acc.samples_per_step == K * B
    assert acc.acc is not None and acc.acc.data_ptr() != acc.grad.data_ptr()
    for tr in (acc, twin):
        tr.cursor.fill_(t0)
    acc.step()
    total = loss = correct = None
    for i in range(K):
        g = twin.compute_grads()
        total = g.clone() if i == 0 else total + g  # ((g_0 + g_1) + g_2), fp32 on the device
        loss = twin.loss.clone() if i == 0 else loss + twin.loss
        correct = twin.correct.clone() if i == 0 else correct + twin.correct
        twin.cursor += 1
    torch.cuda.synchronize()
    got = acc.grad[:N_PARAMS]
    assert torch.equal(got, total), int((got != total).sum())
    assert not torch.equal(got, twin.grad[:N_PARAMS])  # not just the last micro-batch's
    # the twin's unchanged update-from-gradient launch on that sum
    twin.cursor.fill_(t0 + K - 1)  # (that launch bumps the cursor once)
    twin.grad[:N_PARAMS].copy_(total)
    if twin.opt.clips:
        twin._launches()["clip"]()
    twin._sgd(2, from_grad=True, grad_out=False)
    torch.cuda.synchronize()
    _same_trainers(acc, twin, "accumulated step vs the twin's update on the summed gradient")
    assert int(acc.cursor.item()) == t0 + K
    if acc.opt_step is not None:
        assert int(acc.opt_step.item()) == 1 and int(acc.opt_ticket.item()) == 0
        assert torch.equal(acc.clip_norm, twin.clip_norm) and acc.grad_norm() > 0
    st = acc.stats()
    assert st.n == st.samples == 768
    assert st.loss == float(loss.sum()) / 768 and st.accuracy == float(correct.sum()) / 768
    assert sorted(acc.state_extra()) == sorted(twin.state_extra())  # nothing new is checkpointed


# ---- 3. graphs ----
@pytest.mark.parametrize("kw", [SGD, ADAMW_COS_CLIP], ids=["sgd", "adamw-cosine-clip"])
def test_mlp_captured_graphs_equal_eager(kw):
    K, B = 3, 128
    shard = _mnist(4, B)
    clip = dict(clip_grad_norm=0.05) if "optimizer" in kw else {}
    e = _mlp(B, shard=shard, accum_steps=K, **kw, **clip)
    for _ in range(4):
        e.step()
    for unroll in (1, 2):
        a = _mlp(B, shard=shard, accum_steps=K, **kw, **clip)
        a.capture(warmup=0, unroll=unroll)
        a.steps(4)
        torch.cuda.synchronize()
        _same_trainers(a, e, f"accum graph unroll={unroll} vs eager")
        assert torch.equal(a.grad, e.grad) and torch.equal(a.loss, e.loss) and torch.equal(a.correct, e.correct)
        assert int(a.cursor.item()) == 4 * K
        if clip:
            assert torch.equal(a.clip_norm, e.clip_norm) and int(a.opt_step.item()) == 4
        a.drop_graphs()


def test_mlp_set_accum_and_set_world():
    B = 128
    tr = _mlp(B, **SGD)
    assert tr.accum_steps == 1 and tr.acc is None and tr.loss_acc is None and tr.samples_per_step == B
    assert set(tr._launches()) == {"rows", "wgrad", "sgd", "reduce", "update"}  # K = 1: nothing new
    tr.capture(warmup=0, unroll=2)
    tr.set_accum(2)
    assert tr.graph is None and tr.graph_unrolled is None and tr.acc is not None
    assert tr.grad_scale == 1.0 / (2 * B) and tr.samples_per_step == 2 * B
    assert {"acc_store", "acc_add", "acc_fold", "bump"} <= set(tr._launches())
    tr.set_world(4)
    assert tr.accum_steps == 2 and tr.grad_scale == 1.0 / (2 * B * 4)
    tr.step()
    assert int(tr.cursor.item()) == 2 and tr.stats().n == 2 * B
    tr.set_accum(1)
    assert tr.acc is None and tr.grad_scale == 1.0 / (B * 4) and "acc_fold" not in tr._launches()
    tr.step()
    assert int(tr.cursor.item()) == 3 and tr.stats().n == B
    tr.drop_graphs()


# ---- 5. resume (MLP; the ResNet engine's is in the deterministic child) ----
def test_mlp_resume_is_bit_exact():
    K, B = 2, 256
    shard = _mnist(5, B)
    kw = dict(accum_steps=K, **ADAMW_COS_CLIP, clip_grad_norm=0.05)
    a = _mlp(B, shard=shard, **kw)
    for _ in range(2):
        a.step()
    n = a.n_params
    buf = ckfmt.encode(a.get_flat().cpu().numpy(), {"model": a.model_name, "step": 2}, a.mom[:n].cpu().numpy(),
                       a.state_extra())
    meta, params, mom, extra = ckfmt.decode_full(buf)
    assert int(extra["cursor"][0]) == 2 * K and int(extra["opt_step"][0]) == 2
    b = _mlp(B, seed=99, shard=shard, **kw)  # another init: everything must come from the file
    b.set_flat(torch.from_numpy(params))
    b.mom[:n].copy_(torch.from_numpy(mom))
    b.load_state_extra(extra)
    for _ in range(2):
        a.step()
        b.step()
    torch.cuda.synchronize()
    _same_trainers(a, b, "resumed vs straight")
    assert int(a.cursor.item()) == 4 * K and int(a.opt_step.item()) == 4


# ---- 6. refusals ----
def test_refusals():
    from serverless_learn_amd.models.mlp import FusedMLPTrainer
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    class Exchange:
        payload_floats = 1 << 20
        two_shot = inline_sync = False

    for cls in (FusedMLPTrainer, FusedResNetTrainer):
        for bad in (0, -1, 1.5):
            with pytest.raises(ValueError, match="accum_steps"):
                cls(batch=64, device=DEV, accum_steps=bad)
    two = FusedMLPTrainer(batch=64, device=DEV, accum_steps=2)
    with pytest.raises(ValueError, match="accumulation"):
        two.enable_xgmi(Exchange())
    two.enable_xgmi(None)
    one = FusedMLPTrainer(batch=64, device=DEV)
    assert one.acc is None and one.samples_per_step == 64
    one.enable_xgmi(Exchange())
    with pytest.raises(ValueError, match="accumulation"):
        one.set_accum(2)
    assert one.accum_steps == 1 and one.acc is None
    one.set_accum(1)
    one.enable_xgmi(None)
    with pytest.raises(ValueError, match="accum_steps"):
        one.set_accum(0)
    r = FusedResNetTrainer(batch=32, device=DEV)
    assert r.acc is None and r.loss_acc is None and r.samples_per_step == 32 and r.accum_steps == 1
    r.set_accum(2)
    assert r.acc is not None and r.grad_scale == 1.0 / 64 and r.samples_per_step == 64
    r.set_world(2)
    assert r.grad_scale == 1.0 / 128
    r.set_accum(1)
    assert r.acc is None and r.grad_scale == 1.0 / 64


# ---- the runtime worker ----
def test_worker_trains_accumulated_steps_from_graph_chunks():
    """A worker with accum_steps = 2 runs its steps from captured chunks (each step of the unrolled
    graph a whole accumulated step) and ends bit-identical to the bare engine stepped eagerly on
    the same shard; steps count updates and samples count micro-batches."""
    from serverless_learn_amd.models.mlp import FusedMLPTrainer
    from serverless_learn_amd.runtime.local_cluster import LocalCluster, fast_config

    K, B, steps = 2, 256, 24
    c = LocalCluster(fast_config(device=DEV, batch=B, shard_records=8 * B, log_every=8, graph_steps=4,
                                 accum_steps=K, max_steps=steps))
    try:
        w = c.add_worker(sync="none")
        assert c.wait_for(lambda: w.state == "done", 60), (w.state, w.step)
        torch.cuda.synchronize()
        t = w.trainer
        assert w.step == steps and w.samples == steps * K * B and w.graph_chunks > 0
        assert t.accum_steps == K and int(t.cursor.item()) == steps * K
        eng = FusedMLPTrainer(batch=B, device=DEV, accum_steps=K)
        eng.load_shard(t.x, t.y)
        for _ in range(steps):
            eng.step()
        torch.cuda.synchronize()
        _same_trainers(t, eng, "worker vs bare engine")
    finally:
        c.stop()


# ---- 4. / 5. the ResNet engine, in one deterministic-build child ----
@pytest.fixture(scope="module")
def resnet_child():
    env = dict(os.environ, SL_DETERMINISTIC="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "accum_resnet_det.py")], env=env,
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["deterministic_build"], r
    return r


def test_resnet_step_is_the_ordered_sum_of_the_twins_micro_gradients(resnet_child):
    r = resnet_child["twin"]
    print(r)
    assert r["finite"] and r["grad_scale_equal"] and r["samples_per_step"] == 64, r
    assert r["grad_identical"] and r["grad_differs_from_last_micro"], r
    assert r["params_identical"] and r["mom_identical"] and r["shadow_identical"], r
    assert r["running_stats_identical"], r
    assert r["cursor"] == 2 and r["stats_n"] == 64 and r["loss_identical"] and r["accuracy_identical"], r


def test_resnet_bucket_hooks_see_the_folded_sum_in_the_last_micro_batch(resnet_child):
    r = resnet_child["twin"]
    assert r["buckets"] >= 3 and r["hook_cursors"] == [1], r  # the cursor had moved K - 1 = 1 times
    assert r["buckets_tile"] and r["buckets_hold_sum"], r


def test_resnet_input_pipeline_draws_per_micro_batch(resnet_child):
    r = resnet_child["aug"]
    print(r)
    assert r["finite"] and r["grad_identical"] and r["grad_differs_from_last_micro"], r
    assert r["params_identical"] and r["mom_identical"] and r["running_stats_identical"], r
    assert r["aug_out_identical"] and r["mix_out_identical"] and r["cursor"] == 2, r
    assert r["loss_identical"] and r["stats_n"] == 64, r


@pytest.mark.parametrize("case", ["resume", "resume_aug"])
def test_resnet_resume_is_bit_exact(resnet_child, case):
    """``resume``: the fresh trainer has another seed.  ``resume_aug``: shuffle and crop-flip on; the seed
    keys the input pipeline (a setting, not state), so the fresh trainer shares it and starts from other
    weights instead."""
    r = resnet_child[case]
    print(r)
    assert r["finite"] and r["fresh_trainer_differs"], r
    assert r["params_identical"] and r["mom_identical"] and r["v_identical"], r
    assert r["running_stats_identical"] and r["nothing_new_checkpointed"], r
    assert r["cursor"] == [8, 8] and r["opt_step"] == [4, 4], r
