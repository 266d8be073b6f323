"""input_aug_kernel (csrc/kernels/cnn_aux.hip) and the ResNet engine's input pipeline against their
definition, serverless_learn_amd/data/augment.py.  Every comparison is exact: the expected batch is
gathered in u8 space on the host and normalised by the existing input_norm kernel, which shares its
normalise-and-pack arithmetic with input_aug, and the kernel reports each sample's
(record, oy, ox, flip) in ``params_out``."""
import functools

import numpy as np
import pytest
import torch

from serverless_learn_amd.data import augment as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _K():
    from serverless_learn_amd.models.resnet import CIFAR_MEAN, CIFAR_STD
    from serverless_learn_amd.ops import cnn as K

    return K, CIFAR_MEAN, CIFAR_STD


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


def _norm_reference(x_np, lab_np, hw):
    """The existing input_norm kernel on a ready u8 batch (n_batches = 1): (bf16 [B,hw,hw,8], labels)."""
    K, mean, std = _K()
    b = x_np.shape[0]
    xb = torch.from_numpy(np.array(x_np)).to(DEV)  # (a contiguous, writable copy)
    lb = torch.from_numpy(np.array(lab_np)).to(DEV)
    y = torch.full((b, hw, hw, 8), 7.0, dtype=torch.bfloat16, device=DEV)
    lab = torch.full((b,), 255, dtype=torch.uint8, device=DEV)
    K.input_norm(xb, lb, torch.zeros(1, dtype=torch.int32, device=DEV), b, y, lab, mean, std)
    return y, lab


def _expected(x_np, y_np, hw, seed, t, batch, pad, shuffle, augment):
    params = A.batch_params(seed, t, x_np.shape[0], batch, pad, shuffle, augment)
    y, lab = _norm_reference(A.apply(x_np, params, pad), y_np[params[:, 0]], hw)
    return params, y, lab


def _run_aug(xd, yd, hw, seed, t, batch, pad, shuffle, augment):
    K, mean, std = _K()
    y = torch.full((batch, hw, hw, 8), 7.0, dtype=torch.bfloat16, device=DEV)  # channels 3-7 must be written
    lab = torch.full((batch,), 255, dtype=torch.uint8, device=DEV)
    params = torch.full((batch, 4), -1, dtype=torch.int32, device=DEV)
    cursor = torch.full((1,), t, dtype=torch.int32, device=DEV)
    K.input_aug(xd, yd, cursor, batch, y, lab, params, mean, std, seed=seed, shuffle=shuffle, augment=augment,
                pad=pad)
    return y, lab, params


def _check(hw, batch, n, pad, t, seed=0, shuffle=True, augment="crop-flip"):
    x_np, y_np, xd, yd = _shard(n, hw)
    want_p, want_y, want_lab = _expected(x_np, y_np, hw, seed, t, batch, pad, shuffle, augment)
    y, lab, params = _run_aug(xd, yd, hw, seed, t, batch, pad, shuffle, augment)
    torch.cuda.synchronize()
    assert torch.equal(params.cpu(), torch.from_numpy(want_p)), (params.cpu(), want_p)
    assert torch.equal(lab, want_lab)
    assert torch.equal(_bits(y), _bits(want_y))
    return want_p


# ---- the kernel ----
@pytest.mark.parametrize("t", [0, 2, 3, 7])
def test_cifar_batch_both_parts(t):
    """nb = 3: t = 3 is the first batch of epoch 1, t = 7 lies in epoch 2."""
    _check(32, 32, 101, 4, t)


def test_tail_records_are_drawn():
    """Records 96..100 are never reached without the shuffle; some epoch's order holds them early."""
    seen = set()
    for t in range(9):
        seen |= set(A.batch_params(0, t, 101, 32, 4, True, "crop-flip")[:, 0].tolist())
    assert seen & set(range(96, 101)), sorted(seen)
    t = next(t for t in range(9) if set(A.batch_params(0, t, 101, 32, 4, True, "none")[:, 0]) & set(range(96, 101)))
    p = _check(32, 32, 101, 4, t)
    assert set(p[:, 0].tolist()) & set(range(96, 101))


@pytest.mark.parametrize("t", [0, 1, 5])
def test_padding_wider_than_the_image(t):
    """2P + 1 > hw: whole rows and columns of padding; nb = 1, so the epoch is t."""
    p = _check(8, 4, 4, 4, t)
    assert sorted(p[:, 0].tolist()) == [0, 1, 2, 3]


@pytest.mark.parametrize("t", [0, 1, 4])
def test_pixel_tail_and_record_tail(t):
    """400 pixels per image (no multiple of 256 or 64), N % B = 2."""
    _check(20, 3, 5, 2, t)


def test_imagenet_stem_size():
    _check(224, 2, 3, 4, 1)


@pytest.mark.parametrize("t", [0, 3])
def test_flip_only(t):
    p = _check(32, 32, 101, 0, t)
    assert set(p[:, 1].tolist()) == {0} and set(p[:, 2].tolist()) == {0} and set(p[:, 3].tolist()) == {0, 1}


@pytest.mark.parametrize("t", [0, 4])
def test_shuffle_only_is_a_pure_gather(t):
    p = _check(32, 32, 101, 4, t, augment="none")
    assert (p[:, 1:] == (4, 4, 0)).all() and not np.array_equal(p[:, 0], np.arange(32) + (t % 3) * 32)


@pytest.mark.parametrize("t", [0, 4])
def test_augment_only_keeps_the_records(t):
    p = _check(32, 32, 101, 4, t, shuffle=False)
    assert np.array_equal(p[:, 0], np.arange(32) + (t % 3) * 32)


def test_large_cursor():
    """t / nb and the Philox counter in unsigned 32 bits: nb = 2, epoch 1,000,000,005."""
    _check(8, 4, 9, 4, 2_000_000_011)
    _check(8, 4, 9, 4, 2**31 - 1)


def test_seeds_differ_and_calls_repeat():
    x_np, y_np, xd, yd = _shard(101, 32)
    a = _run_aug(xd, yd, 32, 5, 2, 32, 4, True, "crop-flip")
    b = _run_aug(xd, yd, 32, 5, 2, 32, 4, True, "crop-flip")
    c = _run_aug(xd, yd, 32, 6, 2, 32, 4, True, "crop-flip")
    d = _run_aug(xd, yd, 32, 5 + (1 << 32), 2, 32, 4, True, "crop-flip")  # the key's high word counts
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(u) if u.dtype == torch.bfloat16 else u, _bits(v) if v.dtype == torch.bfloat16 else v)
               for u, v in zip(a, b))
    assert not torch.equal(a[2], c[2]) and not torch.equal(a[2], d[2])
    _check(32, 32, 101, 4, 2, seed=5 + (1 << 32))


def test_wrapper_refuses_bad_arguments():
    x_np, y_np, xd, yd = _shard(4, 8)
    with pytest.raises(ValueError):
        _run_aug(xd, yd, 8, 0, 0, 4, 8, True, "crop-flip")
    with pytest.raises(ValueError):
        _run_aug(xd, yd, 8, 0, 0, 4, 4, True, "mixup")


# ---- the engine ----
N_REC, BATCH, SEED = 101, 32, 2


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


ON = dict(augment="crop-flip", shuffle=True)


def _ref(t, **kw):
    kw = {**ON, **kw}
    return torch.from_numpy(A.batch_params(SEED, t, N_REC, BATCH, kw.get("augment_pad", 4), kw["shuffle"],
                                           kw["augment"]))


def test_engine_defaults_launch_no_pipeline(monkeypatch):
    tr = _trainer()
    assert tr.aug_out is None and (tr.augment, tr.augment_pad, tr.shuffle) == ("none", 4, False)

    def boom(*a, **k):
        raise AssertionError("input_aug launched by a default trainer")

    monkeypatch.setattr(tr.K, "input_aug", boom)
    tr.step()
    tr.forward_eval()
    torch.cuda.synchronize()
    x, y = _cifar()
    want, lab = _norm_reference(x[BATCH:2 * BATCH], y[BATCH:2 * BATCH], 32)  # cursor 1: the second plain batch
    assert torch.equal(_bits(tr.x0), _bits(want)) and torch.equal(tr.labels, lab)


def test_engine_refuses_bad_settings():
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    for kw in (dict(augment="mixup"), dict(augment="crop-flip", augment_pad=-1),
               dict(augment="crop-flip", augment_pad=32)):
        with pytest.raises(ValueError, match="augment"):
            FusedResNetTrainer(batch=BATCH, device=DEV, **kw)


def test_engine_eager_steps_cross_epochs():
    tr = _trainer(**ON)
    x, y = _cifar()
    assert tuple(tr.aug_out.shape) == (BATCH, 4) and tr.aug_out.dtype == torch.int32
    for _ in range(7):  # nb = 3: epochs 0, 1 and 2
        t = int(tr.cursor.item())
        tr.step()
        torch.cuda.synchronize()
        want = _ref(t)
        assert torch.equal(tr.aug_out.cpu(), want), t
        assert torch.equal(tr.labels.cpu(), torch.from_numpy(y[want[:, 0].numpy()])), t
        assert np.isfinite(tr.stats().loss), t
    assert t == 6
    _, want_x0, want_lab = _expected(x, y, 32, SEED, t, BATCH, 4, True, "crop-flip")
    assert torch.equal(_bits(tr.x0), _bits(want_x0)) and torch.equal(tr.labels, want_lab)


def test_engine_forward_is_pure():
    tr = _trainer(**ON)
    tr.step()
    tr.compute_grads()
    a, xa = tr.aug_out.clone(), tr.x0.clone()
    tr.compute_grads()
    torch.cuda.synchronize()
    assert torch.equal(a, tr.aug_out) and torch.equal(_bits(xa), _bits(tr.x0))
    assert torch.equal(a.cpu(), _ref(1)) and int(tr.cursor.item()) == 1


def test_engine_graph_replay_draws_fresh_batches():
    tr = _trainer(**ON)
    tr.capture()
    outs = []
    for _ in range(5):
        t = int(tr.cursor.item())
        tr.step()
        torch.cuda.synchronize()
        assert torch.equal(tr.aug_out.cpu(), _ref(t)), t
        outs.append(tr.aug_out.cpu().clone())
    assert tr.graph is not None and int(tr.cursor.item()) == t + 1
    assert all(not torch.equal(outs[i], outs[i + 1]) for i in range(4))


def test_engine_resume_continues_the_stream():
    a = _trainer(**ON)
    for _ in range(3):
        a.step()
    b = _trainer(**ON)
    b.load_state_extra(a.state_extra())
    assert "cursor" in a.state_extra() and not any("aug" in k for k in a.state_extra())
    a.step()
    b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.aug_out, b.aug_out) and torch.equal(a.aug_out.cpu(), _ref(3))
    assert torch.equal(_bits(a.x0), _bits(b.x0)) and torch.equal(a.labels, b.labels)


def test_engine_evaluation_is_plain():
    tr = _trainer(**ON)
    x, y = _cifar()
    for _ in range(4):
        tr.step()
    torch.cuda.synchronize()
    kept = tr.aug_out.clone()
    tr.forward_eval()
    torch.cuda.synchronize()
    b = 4 % (N_REC // BATCH)
    want, lab = _norm_reference(x[b * BATCH:(b + 1) * BATCH], y[b * BATCH:(b + 1) * BATCH], 32)
    assert torch.equal(_bits(tr.x0), _bits(want)) and torch.equal(tr.labels, lab)
    assert torch.equal(tr.aug_out, kept) and int(tr.cursor.item()) == 4
    tr.forward(train=False)  # any forward that is not a training forward
    torch.cuda.synchronize()
    assert torch.equal(_bits(tr.x0), _bits(want)) and torch.equal(tr.aug_out, kept)
    cur = tr.cursor
    st = tr.evaluate(torch.from_numpy(x[:64].copy()), torch.from_numpy(y[:64].copy()))
    torch.cuda.synchronize()
    assert st.samples == 64 and np.isfinite(st.loss)
    assert tr.cursor is cur and int(tr.cursor.item()) == 4 and torch.equal(tr.aug_out, kept)


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
        assert torch.equal(g.aug_out.cpu(), torch.from_numpy(c.last_aug)), t
        assert torch.equal(g.aug_out.cpu(), _ref(t)), t
