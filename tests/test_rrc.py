"""RandomResizedCrop + flip: the integer definition (serverless_learn_amd/data/augment.py rrc_table /
rrc_params / rrc_apply), the refusals, and CPUResNetTrainer's use of it.  The bound of 0.5 is the one
rounding of the definition: at a power-of-two output size the Q8 weights are exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from serverless_learn_amd.data import augment as A


@pytest.mark.parametrize("O", (8, 32))
def test_apply_is_bilinear_interpolation(O):
    x = np.random.default_rng(O).integers(0, 256, size=(3, O, O, 3), dtype=np.uint8)
    boxes = [(0, 0, O, O), (O - 1, 2, 1, 1), (3, 0, 1, O), (0, O - 1, O, 1), (1, 2, O - 3, O // 2), (2, 1, O // 4, O - 2)]
    params = np.array([[j % 3, top, left, h, w, flip, 1, 0] for j, (top, left, h, w) in enumerate(boxes)
                       for flip in (0, 1)], np.int32)
    got = A.rrc_apply(x, params)
    assert got.dtype == np.uint8 and got.shape == (len(params), O, O, 3)
    for row, (rec, top, left, h, w, flip, _, _) in zip(got, params):
        crop = torch.from_numpy(x[rec, top:top + h, left:left + w].astype(np.float64)).permute(2, 0, 1)[None]
        want = F.interpolate(crop, size=(O, O), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
        assert np.abs((row[:, ::-1] if flip else row) - want).max() <= 0.5, (top, left, h, w, flip)
    assert np.array_equal(got[0], x[0]) and np.array_equal(got[1], x[0][:, ::-1])  # the whole image: a copy
    assert np.array_equal(got[1::2], got[0::2][:, :, ::-1])  # flip is the exact mirror


@pytest.mark.parametrize("O,min_scale", ((8, 0.08), (32, 0.08), (12, 0.5), (64, 1.0)))
def test_params_are_a_pure_function_inside_the_image(O, min_scale):
    tab, seed = A.rrc_table(O, min_scale), 9 + (1 << 32)
    p = A.rrc_params(seed, 7, 100, 64, O, True, tab)
    assert p.dtype == np.int32 and p.shape == (64, 8)
    assert np.array_equal(p, A.rrc_params(seed, 7, 100, 64, O, True, tab.copy()))
    assert np.array_equal(p[:, 0], A.batch_params(seed, 7, 100, 64, 0, True, "none")[:, 0])
    rec, top, left, h, w, flip, tries, fb = p.T
    assert (top >= 0).all() and (left >= 0).all() and (h >= 1).all() and (w >= 1).all()
    assert (top + h <= O).all() and (left + w <= O).all()
    assert (tries >= 1).all() and (tries <= 10).all() and set(flip) == {0, 1}
    assert not np.array_equal(p[:, 1:], A.rrc_params(seed, 8, 100, 64, O, True, tab)[:, 1:])  # t is an argument
    if min_scale == 1.0:  # only ratios near 1 fit: redraws and fallbacks happen, every box is the whole image
        assert len(set(tries)) > 2 and fb.any() and (tries[fb == 1] == 10).all() and (h == O).all() and (w == O).all()
    else:  # (ten misses in a row: below 1e-9)
        assert not fb.any()
    miss = A.rrc_params(seed, 7, 100, 64, O, True, np.zeros((256, 256), np.int32))
    assert np.array_equal(miss[:, 1:5], np.tile([0, 0, O, O], (64, 1))) and (miss[:, 6:] == (10, 1)).all()
    assert np.array_equal(miss[:, [0, 5]], p[:, [0, 5]])


def test_cpu_trainer_feeds_the_definition(monkeypatch):
    from serverless_learn_amd.models import resnet as R

    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, size=(9, 8, 8, 3), dtype=np.uint8)
    y = rng.integers(0, 10, size=9, dtype=np.uint8)
    seen = []
    real = R.ref_grads
    monkeypatch.setattr(R, "ref_grads", lambda spec, params, xs, *a, **k: (seen.append(xs), real(spec, params, xs, *a, **k))[1])
    tr = R.CPUResNetTrainer(batch=4, in_hw=8, seed=3, augment="rrc-flip", shuffle=True, rrc_min_scale=0.25)
    tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
    assert tr.last_rrc is None
    for t in range(3):
        tr.step()
        params = A.rrc_params(3, t, 9, 4, 8, True, A.rrc_table(8, 0.25))
        assert np.array_equal(tr.last_rrc, params) and np.array_equal(tr.last_aug, params[:, [0, 1, 2, 5]])
        assert np.array_equal(seen[-1].numpy(), A.rrc_apply(x, params))


def test_refusals_and_config_round_trip(monkeypatch):
    from serverless_learn_amd import config as C
    from serverless_learn_amd.models.resnet import CPUResNetTrainer

    for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rrc_min_scale"):
            C.Config(model="resnet18", augment="rrc-flip", rrc_min_scale=bad)
        with pytest.raises(ValueError, match="rrc_min_scale"):
            CPUResNetTrainer(batch=4, in_hw=8, augment="rrc-flip", rrc_min_scale=bad)
    with pytest.raises(ValueError, match="rrc-flip"):
        CPUResNetTrainer(batch=4, in_hw=10, augment="rrc-flip")  # no multiple of 4
    for model in ("mlp", "simulate"):
        with pytest.raises(ValueError, match="augment"):
            C.Config(model=model, augment="rrc-flip")
    with pytest.raises(ValueError, match="mixup"):
        CPUResNetTrainer(batch=4, in_hw=8, augment="mixup")
    assert C.Config(model="resnet18").rrc_min_scale == 0.08
    for key, value in (("SL_AUGMENT", "rrc-flip"), ("SL_RRC_MIN_SCALE", "0.3"), ("SL_MODEL", "resnet18")):
        monkeypatch.setenv(key, value)
    cfg = C.Config.from_env()
    assert (cfg.augment, cfg.rrc_min_scale) == ("rrc-flip", 0.3)
    ap = C.argparse.ArgumentParser()
    C.add_cli_args(ap)
    cfg = C.from_args(ap.parse_args(["--augment", "rrc-flip", "--rrc-min-scale", "0.5"]))
    assert (cfg.augment, cfg.rrc_min_scale) == ("rrc-flip", 0.5)
