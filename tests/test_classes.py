"""Classifier heads of up to 256 classes, on the CPU: the wide form of the evaluation definition, the
``classes`` setting, the 100-class synthetic dataset, the CPU ResNet trainer with 100 classes and a local
cluster that trains and evaluates on ``synthetic-cifar100``."""
import numpy as np
import pytest
import torch

from serverless_learn_amd.config import Config
from serverless_learn_amd.data import device_synth as DS
from serverless_learn_amd.data.synthetic import decode_shard, make_shard
from serverless_learn_amd.ops import evalmetrics as E

INF, NAN = float("inf"), float("nan")


# ---- eval_reference(wide=True) ----
@pytest.mark.parametrize("ncls", [17, 100, 256])
def test_wide_reference_on_a_hand_made_case(ncls):
    z = torch.zeros(7, ncls)
    lab = torch.zeros(7, dtype=torch.int64)
    loss = torch.tensor([0.5, 1.0, 2.0, 0.25, 3.0, 1.5, 0.125])
    z[0, 3] = z[0, ncls - 1] = 4.0; lab[0] = ncls - 1   # maxima tie, the label at the higher index: pred 3, rank 1
    z[1, 5] = z[1, 16] = 2.0; lab[1] = 5                # ... at the lowest index: pred 5, rank 0
    z[2, 16] = 1.0; lab[2] = ncls                       # a label >= ncls counts as 0: rank 1, pred 16
    z[3, 1] = NAN; lab[3] = 1                           # bad: a NaN logit
    z[4] = -1.0; z[4, ncls - 1] = 0.0; lab[4] = 0       # every class ties but one: rank 1, pred ncls - 1
    loss[5] = INF; lab[5] = 2                           # bad: the loss
    lab[6] = 16                                         # all equal: pred 0, rank 16 (the lower indices are ahead)
    rep = E.eval_reference(z, lab, loss, ncls, 2, wide=True)
    assert (rep.n, rep.bad, rep.top1, rep.topk, rep.k) == (7, 2, 1, 4, 2)
    conf = np.zeros((ncls, ncls), np.int64)
    for l, pr in ((ncls - 1, 3), (5, 5), (0, 16), (0, ncls - 1), (16, 0)):
        conf[l, pr] += 1
    assert np.array_equal(rep.confusion, conf) and rep.confusion.shape == (ncls, ncls)
    assert rep.loss_fix == int((0.5 + 1.0 + 2.0 + 3.0 + 0.125) * (1 << 24))
    assert E.eval_reference(z, lab, loss, ncls, 17, wide=True).topk == 5
    assert E.eval_reference(z, lab, loss, ncls, ncls, wide=True).topk == 5


@pytest.mark.parametrize("ncls", [17, 100, 256])
def test_wide_reports_add(ncls):
    g = torch.Generator().manual_seed(ncls)
    z = torch.randint(-2, 3, (90, ncls), generator=g).float()
    lab = torch.randint(0, ncls, (90,), generator=g)
    loss = torch.rand(90, generator=g) * 4
    z[11, 2] = NAN
    loss[70] = 65536.0
    whole = E.eval_reference(z, lab, loss, ncls, 5, wide=True)
    parts = E.eval_reference(z[:31], lab[:31], loss[:31], ncls, 5, wide=True) \
        + E.eval_reference(z[31:], lab[31:], loss[31:], ncls, 5, wide=True)
    assert whole == parts and whole.bad == 2 and int(whole.confusion.sum()) == 88
    assert len(whole.per_class_recall) == ncls
    # the block form and back
    a = np.zeros(E.acc_len_wide(ncls), np.int64)
    a[:5] = (whole.n, whole.bad, whole.top1, whole.topk, whole.loss_fix)
    a[E.ACC_HEAD:] = whole.confusion.reshape(-1)
    assert E.report_from_acc_wide(a, ncls, 5) == whole


def test_the_narrow_names_are_what_they_were():
    z, lab, loss = torch.zeros(3, 17), torch.zeros(3, dtype=torch.int64), torch.ones(3)
    with pytest.raises(ValueError):
        E.eval_reference(z, lab, loss, 17, 5)
    with pytest.raises(ValueError):
        E.eval_reference(z, lab, loss, 17, 5, wide=False)
    for bad in (0, 257):
        with pytest.raises(ValueError):
            E.eval_reference(torch.zeros(3, 300), lab, loss, bad, 1, wide=True)
        with pytest.raises(ValueError):
            E.acc_len_wide(bad)
    assert (E.MAX_CLASSES, E.ACC_LEN, E.WIDE_CLASSES) == (16, 264, 256)
    assert E.new_acc("cpu").shape == (264,) and E.new_acc_wide("cpu", 100).shape == (8 + 100 * 100,)
    assert E.eval_reference(z[:, :16], lab, loss, 16, 5) == E.eval_reference(z[:, :16], lab, loss, 16, 5, wide=True)


# ---- Config ----
def test_config_classes(monkeypatch):
    assert Config().classes == 0 and Config().n_classes == 10
    assert Config(model="resnet18", dataset="synthetic-cifar").n_classes == 10
    assert Config(model="resnet18", dataset="synthetic-cifar100").n_classes == 100
    assert Config(model="resnet18", dataset="synthetic-cifar100", classes=128).n_classes == 128
    assert Config(model="resnet18", classes=256).n_classes == 256
    assert Config(model="resnet18", classes=1).n_classes == 1
    assert Config(model="mlp", classes=10).n_classes == 10 and Config(model="simulate", classes=10).n_classes == 10
    for kw in (dict(classes=-1), dict(classes=257), dict(classes=2.5), dict(classes=True), dict(model="resnet18", classes=300),
               dict(model="mlp", classes=100), dict(model="mlp", classes=9), dict(model="simulate", classes=100),
               dict(model="mlp", dataset="synthetic-cifar100"), dict(model="simulate", dataset="synthetic-cifar100"),
               dict(model="mlp", dataset="synthetic-cifar100", classes=10)):
        with pytest.raises(ValueError, match="classes"):
            Config(**kw)
    with pytest.raises(ValueError, match="eval_topk"):  # its range stays 1..10
        Config(model="resnet18", classes=100, eval_topk=11)
    monkeypatch.setenv("SL_CLASSES", "100")
    monkeypatch.setenv("SL_MODEL", "resnet18")
    assert Config.from_env().n_classes == 100
    import argparse

    from serverless_learn_amd.config import add_cli_args, from_args

    ap = argparse.ArgumentParser()
    add_cli_args(ap)
    assert from_args(ap.parse_args(["--classes", "37"])).n_classes == 37


# ---- the 100-class dataset ----
def test_kinds_and_prototypes():
    assert DS.KINDS["cifar100"] == DS.KINDS["cifar"] and DS.CLASSES == {"mnist": 10, "cifar": 10, "cifar100": 100}
    p = DS.prototypes("cifar100")
    assert p.shape == (100, 3072) and p.dtype == np.float32 and 0 <= p.min() and p.max() <= 1
    assert len({row.tobytes() for row in p}) == 100
    assert DS.prototypes("cifar").shape == (10, 3072) and DS.prototypes("mnist").shape == (10, 784)
    assert not np.array_equal(p[:10], DS.prototypes("cifar"))
    assert DS.dataset_classes("synthetic-cifar100") == 100 and DS.dataset_classes("synthetic-cifar") == 10
    assert DS.dataset_classes("reference-dummy") == 10


def test_cifar100_shards():
    n = 4096
    a = decode_shard(make_shard(n, 0, 2, seed=3, dataset="synthetic-cifar100"))
    b = decode_shard(make_shard(n, 1, 2, seed=3, dataset="synthetic-cifar100"))
    for hdr, x, y in (a, b):
        assert (hdr["classes"], hdr["height"], hdr["width"], hdr["channels"], hdr["n"]) == (100, 32, 32, 3, n)
        assert x.shape == (n, 3072) and int(y.max()) <= 99 and set(y.tolist()) == set(range(100))
    assert not np.array_equal(a[1], b[1])
    # shards of one seed share the prototypes: the class means of the two shards agree, class by class,
    # far better than the means of different classes do
    def means(x, y):
        return np.stack([x[y == c].astype(np.float64).mean(0) for c in range(100)])

    ma, mb = means(a[1], a[2]), means(b[1], b[2])
    same = np.abs(ma - mb).mean(1)
    other = np.abs(ma - np.roll(mb, 1, axis=0)).mean(1)
    assert same.max() < other.min(), (same.max(), other.min())
    # the other datasets' headers still say ten
    assert decode_shard(make_shard(64, 0, 1, 0, "synthetic-cifar"))[0]["classes"] == 10
    assert decode_shard(make_shard(64, 0, 1, 0, "synthetic-mnist"))[0]["classes"] == 10
    # the numpy generator
    hdr, x, y = decode_shard(make_shard(2048, 0, 1, 0, "synthetic-cifar100", generator="numpy"))
    assert hdr["classes"] == 100 and x.shape == (2048, 3072) and int(y.max()) == 99


def test_native_generator_matches_the_numpy_reference_cifar100():
    """What tests/test_runtime_gpu.py demands of the generators for CIFAR: equal labels, u8 images within 1 and
    fewer than 1 % of them off at all (fp32 rounding ties)."""
    n, seed, first = 300, 5, 1234567
    hdr, x, y = decode_shard(make_shard(n, shard_index=first // n, num_shards=1 + first // n, seed=seed,
                                        dataset="synthetic-cifar100"))
    rx, ry = DS.synth_reference("cifar100", n, seed=seed, first=(first // n) * n)
    assert np.array_equal(y, ry) and int(ry.max()) > 9
    diff = np.abs(x.astype(np.int16) - rx.astype(np.int16))
    assert int(diff.max()) <= 1 and float((diff > 0).mean()) < 0.01, (int(diff.max()), float((diff > 0).mean()))


# ---- the CPU trainer ----
def _cifar100(n, seed=0):
    hdr, x, y = decode_shard(make_shard(n, 0, 1, seed, "synthetic-cifar100"))
    return torch.from_numpy(x.copy()), torch.from_numpy(y.copy())


def test_cpu_trainer_with_100_classes():
    from serverless_learn_amd.models.resnet import CPUResNetTrainer, resnet18_spec

    tr = CPUResNetTrainer(batch=8, classes=100, in_hw=32, lr=0.01)
    assert tr.spec.classes == 100 and tr.n_params == resnet18_spec("cifar", 100, 32).n_flat
    assert dict((n, s) for n, s, _ in tr.layout())["fc.weight"] == [100, 512]
    x, y = _cifar100(24)
    tr.load_shard(x, y)
    before = tr.get_flat()
    for _ in range(2):
        tr.step()
    assert np.isfinite(tr.stats().loss) and not torch.equal(before, tr.get_flat())
    xe, ye = _cifar100(19, seed=1)
    ye[3] = 200  # a label >= classes counts as 0
    rep = tr.evaluate_full(xe, ye, topk=5)
    assert rep.n == 19 and rep.confusion.shape == (100, 100) and int(rep.confusion.sum()) == rep.n - rep.bad
    assert rep.top1 <= rep.topk <= rep.n - rep.bad and rep.k == 5
    assert tr.evaluate_full(xe, ye, topk=100).topk == rep.n - rep.bad
    with pytest.raises(ValueError, match="topk"):
        tr.evaluate_full(xe, ye, topk=101)
    for bad in (0, 257, 2.5):
        with pytest.raises(ValueError, match="classes"):
            CPUResNetTrainer(batch=8, classes=bad, in_hw=32)
    assert CPUResNetTrainer(batch=8, in_hw=32).spec.classes == 10


def test_cpu_trainer_soft_targets_with_100_classes():
    from serverless_learn_amd.models.resnet import CPUResNetTrainer

    tr = CPUResNetTrainer(batch=8, classes=100, in_hw=32, lr=0.01, label_smoothing=0.1, mixup_alpha=0.4)
    tr.load_shard(*_cifar100(16))
    tr.step()
    assert np.isfinite(tr.stats().loss) and tr.last_mix is not None and tr.last_mix.shape == (8, 8)


def test_a_checkpoint_with_another_class_count_is_refused():
    """Nothing new in the checkpoint: n_params follows the spec, and the existing size check of set_flat's copy
    refuses a ten-class checkpoint offered to a 100-class worker before anything is written."""
    from serverless_learn_amd.ckpt import format as ck
    from serverless_learn_amd.models.resnet import CPUResNetTrainer
    from serverless_learn_amd.runtime.worker import Worker

    ten = CPUResNetTrainer(batch=8, in_hw=32)
    data = ck.encode(ten.get_flat().numpy(), {"model": ten.model_name, "step": 3})
    w = Worker("127.0.0.1:0", Config(device="cpu", model="resnet18", classes=100, batch=8))
    w._ensure_trainer()
    assert w.trainer.spec.classes == 100 and w.trainer.n_params != ten.n_params
    assert w.trainer.model_name == ten.model_name  # the name does not tell them apart: the size does
    before = w.trainer.get_flat().clone()
    with pytest.raises(RuntimeError, match="size"):
        w._load_checkpoint(data)
    assert torch.equal(before, w.trainer.get_flat()) and w.step == 0


# ---- the runtime ----
@pytest.mark.slow
def test_two_cpu_workers_train_and_evaluate_on_cifar100(monkeypatch):
    from serverless_learn_amd.runtime.local_cluster import LocalCluster, fast_config
    from serverless_learn_amd.utils.log import Logger

    events = []
    emit = Logger._emit
    monkeypatch.setattr(Logger, "_emit", lambda self, level, event, **f: (events.append((self.role, event, f)),
                                                                         emit(self, level, event, **f)))
    c = LocalCluster(fast_config(dataset="synthetic-cifar100", model="resnet18", batch=8, shard_records=32, lr=0.01,
                                 log_every=1, eval_every=2, eval_records=24, max_steps=2, sync="allreduce"))
    try:
        ws = [c.add_worker(), c.add_worker()]
        assert c.wait_for(lambda: all(w.state == "done" for w in ws), 240), [(w.state, w.step) for w in ws]
        for w in ws:
            assert w.trainer.spec.classes == 100 and w.step == 2 and np.isfinite(w.trainer.stats().loss)
            assert w._eval_shard is not None and w._eval_shard[0].shape == (24, 3072)
        assert torch.equal(ws[0].trainer.params, ws[1].trainer.params)
        evals = [f for role, e, f in events if e == "eval"]
        assert evals and all(f["step"] == 2 and f["n"] == 24 and f["bad"] == 0 for f in evals), evals
        assert not [e for role, e, f in events if e in ("eval_failed", "ingest_class_mismatch")]
    finally:
        c.stop()


@pytest.mark.slow
def test_a_100_class_shard_is_refused_by_a_ten_class_worker(monkeypatch):
    from serverless_learn_amd.runtime.local_cluster import LocalCluster, fast_config
    from serverless_learn_amd.utils.log import Logger

    events = []
    monkeypatch.setattr(Logger, "_emit", lambda self, level, event, **f: events.append((self.role, event, f)))
    c = LocalCluster(fast_config(dataset="synthetic-cifar100", model="resnet18", batch=8, shard_records=32))
    try:
        w = c.add_worker(classes=10, sync="none")
        assert w.cfg.n_classes == 10
        assert c.wait_for(lambda: any(e == "ingest_class_mismatch" for role, e, f in events), 60), events[-5:]
        ev = [f for role, e, f in events if e == "ingest_class_mismatch"]
        assert ev[0]["shard_classes"] == 100 and ev[0]["trainer_classes"] == 10 and ev[0]["file_num"] == 0
        assert not w.has_data.is_set() and w._pending_shard is None and w.files_received == [] and w.step == 0
        assert not [f for role, e, f in events if role == "worker" and e == "received_file"]
    finally:
        c.stop()
