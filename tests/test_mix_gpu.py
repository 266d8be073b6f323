"""input_mix_kernel, the soft-target softmax-CE (csrc/kernels/cnn_aux.hip) and the ResNet engine's
label smoothing / mixup / CutMix against their definition, serverless_learn_amd/data/augment.py.

The input comparisons are exact.  The expected batch is gathered and blended on the host in pixel
units (``mix_apply``: exact multiples of 1/256) and normalised as the kernels' shared core does: one
fused multiply-add per channel, ``round_fp32(v * a + b)`` -- computed here in float64, where the
product and the sum are exact (40 and 39 significant bits), and rounded once to fp32, then to bf16.
The soft-target loss is compared with a float64 torch reference built from ``soft_targets``, with
the bounds tests/test_cnn_gpu.py uses for the one-hot kernel; `correct` is the argmax against each
sample's own label, which under mixing is a diagnostic and not an accuracy."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from serverless_learn_amd.data import augment as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = {"mixup": (0.4, 0.0), "cutmix": (0.0, 1.0), "both": (0.4, 1.0)}


def _K():
    from serverless_learn_amd.models.resnet import CIFAR_MEAN, CIFAR_STD
    from serverless_learn_amd.ops import cnn as K

    return K, CIFAR_MEAN, CIFAR_STD


def rel(a, b):
    """The norm-wise measure of tests/test_cnn_gpu.py."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


@functools.lru_cache(maxsize=None)
def _shard(n, hw):
    """(x u8 [n,hw,hw,3], labels u8 [n]) on the host (read-only) and on the device."""
    rng = np.random.default_rng(1000 * n + hw)
    x = rng.integers(0, 256, size=(n, hw, hw, 3), dtype=np.uint8)
    y = rng.integers(0, 10, size=n, dtype=np.uint8)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y, torch.from_numpy(x.copy()).to(DEV), torch.from_numpy(y.copy()).to(DEV)


def _bits(t):
    return t.view(torch.int16)


def _norm_bits(v):
    """bf16 bits [B,H,W,8] (int16, on the host) of pixel-unit values v [B,H,W,3] float32."""
    _, mean, std = _K()
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    a = (np.float32(1) / (np.float32(255) * s)).astype(np.float32)  # the launcher's fp32 arithmetic
    b = (-m / s).astype(np.float32)
    f = (v.astype(np.float64) * a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
    out = torch.zeros(*v.shape[:3], 8, dtype=torch.bfloat16)
    out[..., :3] = torch.from_numpy(f).to(torch.bfloat16)
    return _bits(out)


def _expected(x_np, y_np, hw, seed, t, batch, pad, shuffle, augment, ma, ca):
    params = A.batch_params(seed, t, x_np.shape[0], batch, pad, shuffle, augment)
    mix = A.mix_params(seed, t, batch, hw, hw, ma, ca)
    v = A.mix_apply(A.apply(x_np, params, pad), mix)
    return params, mix, _norm_bits(v), y_np[params[:, 0]]


def _run_mix(xd, yd, hw, seed, t, batch, pad, shuffle, augment, ma, ca, table=None):
    K, mean, std = _K()
    y = torch.full((batch, hw, hw, 8), 7.0, dtype=torch.bfloat16, device=DEV)  # channels 3-7 must be written
    lab = torch.full((batch,), 255, dtype=torch.uint8, device=DEV)
    params = torch.full((batch, 4), -1, dtype=torch.int32, device=DEV)
    mix = torch.full((batch, 8), -1, dtype=torch.int32, device=DEV)
    cursor = torch.full((1,), t, dtype=torch.int32, device=DEV)
    tab = torch.from_numpy(A.mix_tables(ma, ca) if table is None else table).to(DEV)
    K.input_mix(xd, yd, cursor, batch, y, lab, params, mix, tab, mean, std, seed=seed, shuffle=shuffle,
                augment=augment, pad=pad, mixup=ma > 0, cutmix=ca > 0)
    return y, lab, params, mix


def _run_aug(xd, yd, hw, seed, t, batch, pad, shuffle, augment):
    K, mean, std = _K()
    y = torch.full((batch, hw, hw, 8), 7.0, dtype=torch.bfloat16, device=DEV)
    lab = torch.full((batch,), 255, dtype=torch.uint8, device=DEV)
    params = torch.full((batch, 4), -1, dtype=torch.int32, device=DEV)
    cursor = torch.full((1,), t, dtype=torch.int32, device=DEV)
    K.input_aug(xd, yd, cursor, batch, y, lab, params, mean, std, seed=seed, shuffle=shuffle, augment=augment,
                pad=pad)
    return y, lab, params


def _check(hw, batch, n, pad, t, mode, seed=0, shuffle=True, augment="crop-flip"):
    ma, ca = MODES[mode]
    x_np, y_np, xd, yd = _shard(n, hw)
    want_p, want_m, want_y, want_lab = _expected(x_np, y_np, hw, seed, t, batch, pad, shuffle, augment, ma, ca)
    y, lab, params, mix = _run_mix(xd, yd, hw, seed, t, batch, pad, shuffle, augment, ma, ca)
    torch.cuda.synchronize()
    assert torch.equal(params.cpu(), torch.from_numpy(want_p)), (t, params.cpu(), want_p)
    assert torch.equal(mix.cpu(), torch.from_numpy(want_m)), (t, mix.cpu(), want_m)
    assert torch.equal(lab.cpu(), torch.from_numpy(want_lab.copy()))
    got = _bits(y).cpu()
    bad = (got != want_y).nonzero()
    assert bad.numel() == 0, (t, mode, bad[:4], got[tuple(bad[0])], want_y[tuple(bad[0])])
    return want_m


# ---- the input kernel ----
@pytest.mark.parametrize("mode", list(MODES))
def test_cifar_batch_across_epochs(mode):
    """nb = 3: t = 3 is the first batch of epoch 1, t = 7 lies in epoch 2."""
    seen = set()
    for t in (0, 2, 3, 7):
        seen.add(int(_check(32, 32, 101, 4, t, mode)[0, 3]))
    assert seen <= {1, 2} and (mode != "mixup" or seen == {1}) and (mode != "cutmix" or seen == {2})


def test_both_modes_occur():
    x_np, y_np, xd, yd = _shard(101, 32)
    ts = [next(t for t in range(64) if A.mix_params(0, t, 32, 32, 32, 0.4, 1.0)[0, 3] == m) for m in (1, 2)]
    assert {int(_check(32, 32, 101, 4, t, "both")[0, 3]) for t in ts} == {1, 2}


@pytest.mark.parametrize("mode", list(MODES))
def test_padding_wider_than_the_image_and_a_large_cursor(mode):
    """2P + 1 > hw; nb = 1, so the epoch is t; t / nb and the Philox counters in unsigned 32 bits."""
    for t in (0, 1, 5, 2_000_000_011, 2**31 - 1):
        _check(8, 4, 4, 4, t, mode)


@pytest.mark.parametrize("mode", list(MODES))
def test_pixel_tail_record_tail_and_odd_batch(mode):
    """400 pixels per image (no multiple of 256 or 64), N % B = 2, B - 1 = 2 rotations."""
    for t in (0, 1, 4, 2_000_000_011):
        _check(20, 3, 5, 2, t, mode)


@pytest.mark.parametrize("mode", list(MODES))
def test_imagenet_stem_size(mode):
    _check(224, 2, 3, 4, 1, mode)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kw", [dict(shuffle=False, augment="none"), dict(shuffle=True, augment="none"),
                                dict(shuffle=False, augment="crop-flip")])
def test_parts_of_the_pipeline_off(mode, kw):
    for t in (0, 4):
        _check(32, 32, 101, 4, t, mode, **kw)
    _check(20, 3, 5, 2, 3, mode, **kw)


def test_seeds_differ_and_calls_repeat():
    x_np, y_np, xd, yd = _shard(101, 32)
    run = lambda seed: _run_mix(xd, yd, 32, seed, 2, 32, 4, True, "crop-flip", 0.4, 1.0)  # noqa: E731
    a, b, c, d = run(5), run(5), run(6), run(5 + (1 << 32))  # the key's high word counts
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(u) if u.dtype == torch.bfloat16 else u, _bits(v) if v.dtype == torch.bfloat16 else v)
               for u, v in zip(a, b))
    assert not torch.equal(_bits(a[0]), _bits(c[0])) and not torch.equal(_bits(a[0]), _bits(d[0]))
    _check(32, 32, 101, 4, 2, "both", seed=5 + (1 << 32))


# ---- device against device: no reference arithmetic ----
@pytest.mark.parametrize("mode", list(MODES))
def test_a_table_that_mixes_nothing_gives_input_aug(mode):
    """All k = 256 (lambda 1) and all c = 0 (an empty box): bit for bit what input_aug writes."""
    ma, ca = MODES[mode]
    x_np, y_np, xd, yd = _shard(101, 32)
    table = np.full((2, A.MIX_L), 256, np.int32)
    for t in (0, 5):
        y, lab, params, mix = _run_mix(xd, yd, 32, 0, t, 32, 4, True, "crop-flip", ma, ca, table=table)
        y0, lab0, params0 = _run_aug(xd, yd, 32, 0, t, 32, 4, True, "crop-flip")
        torch.cuda.synchronize()
        assert torch.equal(_bits(y), _bits(y0)) and torch.equal(lab, lab0) and torch.equal(params, params0)
        assert (mix[:, 1] == 0).all() and (mix[:, 0] != torch.arange(32, device=DEV)).all()


@pytest.mark.parametrize("mode", list(MODES))
def test_identical_images_stay_unmixed(mode):
    """A shard of one image under any lambda or box (shuffled records, no crop): the plain image."""
    K, mean, std = _K()
    ma, ca = MODES[mode]
    x_np, y_np, _, _ = _shard(101, 32)
    xd = torch.from_numpy(np.broadcast_to(x_np[7], (11, 32, 32, 3)).copy()).to(DEV)
    yd = torch.from_numpy(y_np[:11].copy()).to(DEV)
    want = torch.empty(4, 32, 32, 8, dtype=torch.bfloat16, device=DEV)
    K.input_norm(xd, yd, torch.zeros(1, dtype=torch.int32, device=DEV), 4, want,
                 torch.empty(4, dtype=torch.uint8, device=DEV), mean, std)
    for t in (0, 1, 2, 3):
        y, _, _, mix = _run_mix(xd, yd, 32, 9, t, 4, 4, True, "none", ma, ca)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y), _bits(want)), (t, mix[0])


def test_wrapper_refuses_bad_arguments():
    x_np, y_np, xd, yd = _shard(4, 8)
    with pytest.raises(ValueError):
        _run_mix(xd, yd, 8, 0, 0, 4, 8, True, "crop-flip", 0.4, 0.0)
    with pytest.raises(ValueError):
        _run_mix(xd, yd, 8, 0, 0, 4, 4, True, "mixup", 0.4, 0.0)
    with pytest.raises(ValueError):
        _run_mix(xd, yd, 8, 0, 0, 4, 4, True, "crop-flip", 0.0, 0.0, table=A.mix_tables(1.0, 1.0))
    with pytest.raises(ValueError):
        _run_mix(xd[:1], yd[:1], 8, 0, 0, 1, 4, True, "crop-flip", 0.4, 0.0)


# ---- the soft-target loss ----
def _ce_inputs():
    g = torch.Generator().manual_seed(2)
    z = (torch.randn(37, 10, generator=g) * 3).to(DEV)
    lab = torch.randint(0, 10, (37,), generator=g, dtype=torch.uint8).to(DEV)
    return z, lab


def _ce_mix(kind):
    """int32 [37, 8] rows as input_mix writes them, with num = 0 and num = den among them."""
    m = np.zeros((37, 8), np.int32)
    m[:, 0] = (np.arange(37) + 5) % 37
    if kind == "mixup":
        m[:, 1], m[:, 2], m[:, 3] = (np.arange(37) * 7) % 257, 256, 1
        m[3, 1], m[4, 1] = 0, 256
    else:
        m[:, 1], m[:, 2], m[:, 3] = (np.arange(37) * 29) % 1025, 1024, 2
        m[3, 1], m[4, 1] = 0, 1024
        m[:, 4:] = (1, 2, 3, 4)
    return m


def _ce_run(fn, z, lab, **kw):
    loss = torch.full((37,), 9.0, device=DEV)
    corr = torch.full((37,), 9.0, device=DEV)
    dz = torch.full((37, 16), 9.0, dtype=torch.bfloat16, device=DEV)
    db = torch.zeros(10, device=DEV)
    fn(z, lab, loss, corr, dz, db, 0.5, **kw)
    torch.cuda.synchronize()
    return loss, corr, dz, db


def _soft_ce_checks():
    """Every soft-CE assertion (also run under the deterministic build, in a child process)."""
    from serverless_learn_amd.ops import _native as N

    K, _, _ = _K()
    z, lab = _ce_inputs()
    det = bool(N.lib().sl_deterministic())
    for eps in (0.0, 0.1):
        for kind in (None, "mixup", "cutmix"):
            m = None if kind is None else _ce_mix(kind)
            md = None if m is None else torch.from_numpy(m).to(DEV)
            loss, corr, dz, db = _ce_run(K.softmax_ce_soft, z, lab, mix=md, eps=eps)
            q = torch.from_numpy(A.soft_targets(lab.cpu().numpy(), m, eps, 10))
            assert float((q.sum(1) - 1).abs().max()) < 1e-12
            zr = z.double().cpu().requires_grad_(True)
            want = torch.logsumexp(zr, 1) - (q * zr).sum(1)
            (want.sum() * 0.5).backward()
            figs = (rel(loss, want), rel(dz[:, :10], zr.grad), rel(db, zr.grad.sum(0)))
            print(f"eps {eps} mix {kind}: loss rel {figs[0]:.2e} dz rel {figs[1]:.2e} dbias rel {figs[2]:.2e}")
            assert figs[0] < 1e-4, (eps, kind, figs)
            assert figs[1] < 1e-2 and float(dz[:, 10:].float().abs().max()) == 0, (eps, kind, figs)
            assert figs[2] < 1e-4, (eps, kind, figs)
            assert torch.equal(corr.cpu(), (z.argmax(1) == lab.long()).float().cpu())  # the own label
    hard = _ce_run(K.softmax_ce, z, lab)
    soft = _ce_run(K.softmax_ce_soft, z, lab, mix=None, eps=0.0)
    assert torch.equal(hard[0], soft[0]) and torch.equal(hard[1], soft[1])
    assert torch.equal(_bits(hard[2]), _bits(soft[2]))
    if det:
        assert torch.equal(hard[3], soft[3])
    else:
        assert rel(soft[3], hard[3]) < 1e-6
    return det


def test_soft_ce_against_float64():
    _soft_ce_checks()


def test_soft_ce_in_the_deterministic_build():
    """A process loads one kernel library: the same checks in a child process with the
    fixed-point bias-gradient epilogue, where dbias equals the one-hot kernel's bit for bit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SL_DETERMINISTIC="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=root, capture_output=True,
                         text=True, timeout=170)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2000:])
    assert json.loads(out.stdout.strip().splitlines()[-1]) == {"deterministic_build": True, "ok": True}


def test_soft_ce_wrapper_refuses_bad_smoothing():
    K, _, _ = _K()
    z, lab = _ce_inputs()
    for eps in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            _ce_run(K.softmax_ce_soft, z, lab, eps=eps)


# ---- the engine ----
N_REC, BATCH, SEED, EPS = 101, 32, 2, 0.1
ON = dict(augment="crop-flip", shuffle=True, label_smoothing=EPS, mixup_alpha=0.4, cutmix_alpha=1.0)


@functools.lru_cache(maxsize=None)
def _cifar():
    from serverless_learn_amd.data.synthetic import make_cifar_like

    x, y = make_cifar_like(N_REC, seed=5)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _trainer(**kw):
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    x, y = _cifar()
    tr = FusedResNetTrainer(batch=BATCH, device=DEV, seed=SEED, **kw)
    tr.load_shard(torch.from_numpy(x.copy()), torch.from_numpy(y.copy()))
    return tr


def _ref(t):
    return (torch.from_numpy(A.batch_params(SEED, t, N_REC, BATCH, 4, True, "crop-flip")),
            torch.from_numpy(A.mix_params(SEED, t, BATCH, 32, 32, 0.4, 1.0)))


def test_engine_defaults_launch_neither_kernel(monkeypatch):
    tr = _trainer()
    assert tr.aug_out is None and tr.mix_out is None
    assert (tr.label_smoothing, tr.mixup_alpha, tr.cutmix_alpha) == (0.0, 0.0, 0.0)

    def boom(*a, **k):
        raise AssertionError("a mix / soft-target kernel launched by a default trainer")

    monkeypatch.setattr(tr.K, "input_mix", boom)
    monkeypatch.setattr(tr.K, "softmax_ce_soft", boom)
    tr.step()
    tr.forward_eval()
    torch.cuda.synchronize()
    assert np.isfinite(tr.stats().loss)


def test_engine_refuses_bad_settings():
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    for kw in (dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(mixup_alpha=-1.0),
               dict(mixup_alpha=float("inf")), dict(cutmix_alpha=float("nan")), dict(cutmix_alpha=-2.0)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            FusedResNetTrainer(batch=BATCH, device=DEV, **kw)
    with pytest.raises(ValueError, match="batch"):
        FusedResNetTrainer(batch=1, device=DEV, mixup_alpha=0.2)
    with pytest.raises(ValueError, match="augment"):
        FusedResNetTrainer(batch=BATCH, device=DEV, augment="mixup")


def _check_loss(tr):
    """loss and dlogits of the last training forward against the engine's own logits."""
    from serverless_learn_amd.models.resnet_engine import LOGIT_LD

    mix = tr.mix_out.cpu().numpy() if tr.mix_out is not None else None
    q = torch.from_numpy(A.soft_targets(tr.labels.cpu().numpy(), mix, tr.label_smoothing, 10))
    z = tr.logits.double().cpu()
    want = torch.logsumexp(z, 1) - (q * z).sum(1)
    assert rel(tr.loss, want) < 1e-4, rel(tr.loss, want)
    loss, corr = torch.zeros(BATCH, device=DEV), torch.zeros(BATCH, device=DEV)
    dz = torch.zeros(BATCH, LOGIT_LD, dtype=torch.bfloat16, device=DEV)
    tr.K.softmax_ce_soft(tr.logits, tr.labels, loss, corr, dz, None, tr.grad_scale, mix=tr.mix_out,
                         eps=tr.label_smoothing)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dz), _bits(tr.dlogits.view(BATCH, LOGIT_LD))) and torch.equal(loss, tr.loss)
    assert torch.equal(corr, tr.correct)


def test_engine_eager_steps_cross_epochs():
    tr = _trainer(**ON)
    x, y = _cifar()
    assert tuple(tr.aug_out.shape) == (BATCH, 4) and tuple(tr.mix_out.shape) == (BATCH, 8)
    assert tr.mix_out.dtype == torch.int32
    modes = set()
    for _ in range(7):  # nb = 3: epochs 0, 1 and 2
        t = int(tr.cursor.item())
        tr.step()
        torch.cuda.synchronize()
        want_p, want_m = _ref(t)
        assert torch.equal(tr.aug_out.cpu(), want_p) and torch.equal(tr.mix_out.cpu(), want_m), t
        assert torch.equal(tr.labels.cpu(), torch.from_numpy(y[want_p[:, 0].numpy()])), t
        assert np.isfinite(tr.stats().loss), t
        modes.add(int(want_m[0, 3]))
    assert t == 6 and modes == {1, 2}
    _, _, want_x0, want_lab = _expected(x, y, 32, SEED, t, BATCH, 4, True, "crop-flip", 0.4, 1.0)
    assert torch.equal(_bits(tr.x0).cpu(), want_x0) and torch.equal(tr.labels.cpu(), torch.from_numpy(want_lab.copy()))
    _check_loss(tr)


@pytest.mark.parametrize("kw", [dict(label_smoothing=EPS), dict(mixup_alpha=0.4), dict(cutmix_alpha=1.0)])
def test_engine_each_setting_alone(kw, monkeypatch):
    tr = _trainer(**kw)
    x, y = _cifar()
    if "label_smoothing" in kw:  # smoothing alone keeps today's input kernel
        assert tr.aug_out is None and tr.mix_out is None
        monkeypatch.setattr(tr.K, "input_mix", lambda *a, **k: pytest.fail("input_mix launched"))
    for _ in range(2):
        tr.step()
    torch.cuda.synchronize()
    if tr.mix_out is not None:
        ma, ca = kw.get("mixup_alpha", 0.0), kw.get("cutmix_alpha", 0.0)
        want_p, want_m, want_x0, _ = _expected(x, y, 32, SEED, 1, BATCH, 4, False, "none", ma, ca)
        assert torch.equal(tr.aug_out.cpu(), torch.from_numpy(want_p))
        assert torch.equal(tr.mix_out.cpu(), torch.from_numpy(want_m)) and torch.equal(_bits(tr.x0).cpu(), want_x0)
    _check_loss(tr)


def test_engine_graph_replay_draws_fresh_batches():
    tr = _trainer(**ON)
    tr.capture()
    outs = []
    for _ in range(5):
        t = int(tr.cursor.item())
        tr.step()
        torch.cuda.synchronize()
        want_p, want_m = _ref(t)
        assert torch.equal(tr.aug_out.cpu(), want_p) and torch.equal(tr.mix_out.cpu(), want_m), t
        outs.append(tr.mix_out.cpu().clone())
    assert tr.graph is not None and int(tr.cursor.item()) == t + 1
    assert any(not torch.equal(outs[i], outs[i + 1]) for i in range(4))
    _check_loss(tr)


def test_engine_resume_continues_the_stream():
    a = _trainer(**ON)
    for _ in range(3):
        a.step()
    b = _trainer(**ON)
    b.load_state_extra(a.state_extra())
    assert set(a.state_extra()) == set(_trainer().state_extra())  # no new checkpoint key
    assert len(a.buffers()) == len(_trainer().buffers())
    a.step()
    b.step()
    torch.cuda.synchronize()
    want_p, want_m = _ref(3)
    assert torch.equal(a.aug_out, b.aug_out) and torch.equal(a.aug_out.cpu(), want_p)
    assert torch.equal(a.mix_out, b.mix_out) and torch.equal(a.mix_out.cpu(), want_m)
    assert torch.equal(_bits(a.x0), _bits(b.x0)) and torch.equal(a.labels, b.labels)


def test_engine_evaluation_is_plain(monkeypatch):
    K, mean, std = _K()
    tr = _trainer(**ON)
    x, y = _cifar()
    for _ in range(4):
        tr.step()
    torch.cuda.synchronize()
    kept_a, kept_m = tr.aug_out.clone(), tr.mix_out.clone()
    monkeypatch.setattr(tr.K, "input_mix", lambda *a, **k: pytest.fail("input_mix launched by an evaluation path"))
    monkeypatch.setattr(tr.K, "softmax_ce_soft", lambda *a, **k: pytest.fail("soft loss in an evaluation path"))
    b = 4 % (N_REC // BATCH)
    xb = torch.from_numpy(x[b * BATCH:(b + 1) * BATCH].copy()).to(DEV)
    lb = torch.from_numpy(y[b * BATCH:(b + 1) * BATCH].copy()).to(DEV)
    want = torch.empty(BATCH, 32, 32, 8, dtype=torch.bfloat16, device=DEV)
    K.input_norm(xb, lb, torch.zeros(1, dtype=torch.int32, device=DEV), BATCH, want,
                 torch.empty(BATCH, dtype=torch.uint8, device=DEV), mean, std)
    for fwd in (tr.forward_eval, lambda: tr.forward(train=False)):
        fwd()
        torch.cuda.synchronize()
        assert torch.equal(_bits(tr.x0), _bits(want)) and torch.equal(tr.labels, lb)
        assert torch.equal(tr.aug_out, kept_a) and torch.equal(tr.mix_out, kept_m) and int(tr.cursor.item()) == 4
        z = tr.logits.double()
        one_hot = torch.logsumexp(z, 1) - z.gather(1, tr.labels.long()[:, None])[:, 0]
        assert rel(tr.loss, one_hot) < 1e-4  # one-hot, unsmoothed
    st = tr.evaluate(torch.from_numpy(x[:64].copy()), torch.from_numpy(y[:64].copy()))
    torch.cuda.synchronize()
    assert st.samples == 64 and np.isfinite(st.loss)
    assert int(tr.cursor.item()) == 4 and torch.equal(tr.aug_out, kept_a) and torch.equal(tr.mix_out, kept_m)


def test_cpu_and_gpu_trainers_draw_the_same_batches():
    from serverless_learn_amd.models.resnet import CPUResNetTrainer

    x, y = _cifar()
    g = _trainer(**ON)
    c = CPUResNetTrainer(batch=BATCH, seed=SEED, **ON)
    c.load_shard(torch.from_numpy(x.copy()), torch.from_numpy(y.copy()))
    for t in range(4):
        g.step()
        c.step()
        torch.cuda.synchronize()
        want_p, want_m = _ref(t)
        assert torch.equal(g.aug_out.cpu(), torch.from_numpy(c.last_aug)) and torch.equal(g.aug_out.cpu(), want_p), t
        assert torch.equal(g.mix_out.cpu(), torch.from_numpy(c.last_mix)) and torch.equal(g.mix_out.cpu(), want_m), t


if __name__ == "__main__":  # the child process of test_soft_ce_in_the_deterministic_build
    print(json.dumps({"deterministic_build": _soft_ce_checks(), "ok": True}))
