"""TrivialAugment Wide: the integer definition (serverless_learn_amd/data/augment.py ta_table /
ta_params / ta_apply), the refusals, and CPUResNetTrainer's use of it.

Solarize at bin 0 has threshold 255, so by its definition (``a < th ? a : 255 - a``, torchvision's
rule) a pixel at 255 becomes 0 and every other pixel stays: the bin-0 case asserts exactly that."""
import ctypes

import numpy as np
import pytest
import torch

from serverless_learn_amd.data import augment as A

OPS = {name: i for i, name in enumerate(A.TA_OPS)}


def _image(h=9, w=7, seed=0):
    a = np.random.default_rng(seed).integers(0, 256, size=(1, h, w, 3), dtype=np.uint8)
    a[0, 2, 3] = (255, 0, 255)  # both ends of the range occur
    return a


def _one(a, op, b=0, neg=0):
    return A.ta_apply(a, np.array([[op, b, neg, 0]], np.int32))[0]


@pytest.mark.parametrize("op", range(12))
@pytest.mark.parametrize("neg", (0, 1))
def test_bin_zero_is_the_input(op, neg):
    a = _image()
    want = a[0].copy()
    if op == OPS["Solarize"]:
        assert (want == 255).any()
        want[want == 255] = 0
    assert np.array_equal(_one(a, op, 0, neg), want)
    assert np.array_equal(_one(a, OPS["Identity"], 17, neg), a[0])


@pytest.mark.parametrize("neg,k", ((0, 1), (1, -1)))
def test_rotate_by_a_quarter_turn(neg, k):
    a = _image(6, 6)
    assert tuple(A.ta_table()[OPS["Rotate"], 20, neg, :6]) in {(0, -65536, 0, 65536, 0, 0), (0, 65536, 0, -65536, 0, 0)}
    assert np.array_equal(_one(a, OPS["Rotate"], 20, neg), np.rot90(a[0], k))


@pytest.mark.parametrize("neg", (0, 1))
def test_translate_is_a_shifted_slice(neg):
    a = _image(9, 11)
    want = np.zeros((2, 9, 11, 3), np.uint8)  # bin 3: rint(3.2) = 3 pixels, right / down, or left / up
    if neg:
        want[0][:, :-3], want[1][:-3] = a[0][:, 3:], a[0][3:]
    else:
        want[0][:, 3:], want[1][3:] = a[0][:, :-3], a[0][:-3]
    assert np.array_equal(_one(a, OPS["TranslateX"], 3, neg), want[0])
    assert np.array_equal(_one(a, OPS["TranslateY"], 3, neg), want[1])
    assert not _one(a, OPS["TranslateX"], 30, neg).any()  # 32 pixels: out of an 11-wide image


def test_constant_and_posterized_images():
    flat = np.full((1, 20, 20, 3), 93, np.uint8)
    for op in (OPS["AutoContrast"], OPS["Equalize"], OPS["Contrast"], OPS["Sharpness"], OPS["Color"]):
        assert np.array_equal(_one(flat, op, 30, 1), flat[0]), op
    a = _image(20, 20)
    assert np.array_equal(_one(a, OPS["Posterize"], 30), a[0] & 0xC0)  # 2 bits left
    assert np.array_equal(_one(a, OPS["Solarize"], 30), 255 - a[0])
    two = np.where(np.arange(400).reshape(1, 20, 20, 1) % 4 == 0, 40, 200).astype(np.uint8).repeat(3, axis=3)
    # 100 pixels at 40, 300 at 200: step = 100 // 255 = 0 leaves it alone; AutoContrast spreads it
    assert np.array_equal(_one(two, OPS["Equalize"]), two[0])
    assert set(np.unique(_one(two, OPS["AutoContrast"]))) == {0, 255}


def test_draws_reach_every_op_bin_and_sign():
    p = np.concatenate([A.ta_params(7, t, 1024) for t in range(4)])
    assert p.dtype == np.int32 and not p[:, 3].any()
    assert set(p[:, 0]) == set(range(14)) and set(p[:, 1]) == set(range(31)) and set(p[:, 2]) == {0, 1}
    assert np.bincount(p[:, 0]).min() > 4096 / 14 * 0.7


def test_refusals():
    from serverless_learn_amd.config import Config
    from serverless_learn_amd.models.resnet import CPUResNetTrainer
    from serverless_learn_amd.ops import _native as N

    with pytest.raises(ValueError, match="auto_augment"):
        CPUResNetTrainer(batch=4, in_hw=8, auto_augment="rand")
    with pytest.raises(ValueError, match="auto_augment"):
        CPUResNetTrainer(batch=4, stem="imagenet", auto_augment="trivial-wide")  # 224 x 224 > 4096 pixels
    with pytest.raises(ValueError, match="auto_augment"):
        Config(model="resnet18", auto_augment="rand")
    for model in ("mlp", "simulate"):
        with pytest.raises(ValueError, match="auto_augment"):
            Config(model=model, auto_augment="trivial-wide")
    assert Config(model="resnet18", auto_augment="trivial-wide").auto_augment == "trivial-wide"
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)  # (never read: every call below is refused before a launch)
    ok = dict(n=4, batch=4, H=8, W=8, force=-1, ptr=a)
    for bad in (dict(H=65, W=64), dict(batch=0), dict(n=3), dict(ptr=None), dict(force=14), dict(force=31 << 8)):
        k = dict(ok, **bad)
        rc = N.lib().sl_input_ta(k["ptr"], a, a, k["n"], k["batch"], k["H"], k["W"], 4, 3, 0, a, a, a, a, a, k["force"],
                                 None)
        assert rc != 0, bad


def test_cpu_trainer_feeds_the_definition(monkeypatch):
    from serverless_learn_amd.models import resnet as R

    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, size=(9, 8, 8, 3), dtype=np.uint8)
    y = rng.integers(0, 10, size=9, dtype=np.uint8)
    seen = []
    real = R.ref_grads
    monkeypatch.setattr(R, "ref_grads", lambda spec, params, xs, *a, **k: (seen.append(xs), real(spec, params, xs, *a, **k))[1])
    tr = R.CPUResNetTrainer(batch=4, in_hw=8, seed=3, augment="crop-flip", shuffle=True, auto_augment="trivial-wide")
    tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
    assert tr.ta_out is None
    for t in range(3):
        tr.step()
        params = A.batch_params(3, t, 9, 4, 4, True, "crop-flip")
        ta = A.ta_params(3, t, 4)
        assert np.array_equal(tr.ta_out, ta) and np.array_equal(tr.last_aug, params)
        assert np.array_equal(seen[-1].numpy(), A.ta_apply(A.apply(x, params, 4), ta))
