#!/usr/bin/env python
"""What the ResNet engine's input pipeline costs (profiles/r13_input), and what label smoothing,
mixup and CutMix add to it (profiles/r14_mix).

Four measurements, each a process of its own so that each runs under its own time limit:

    timeout -k 10 300 python scripts/aug_probe.py kernel --out profiles/r13_input && \\
    timeout -k 10 600 python scripts/aug_probe.py step --out profiles/r13_input
    timeout -k 10 300 python scripts/aug_probe.py mix --out profiles/r14_mix && \\
    timeout -k 10 900 python scripts/aug_probe.py mix_step --out profiles/r14_mix

kernel  input_norm_kernel and input_aug_kernel with each combination of parts on (aug_off: neither,
        which no trainer launches -- the cost of the per-image layout alone), B = 1024 images
        of 32x32 out of a 16,384-record shard: device events around 200 launches of each,
        interleaved, several rounds.  Reports microseconds per launch and the GB/s implied by
        3 + 16 bytes per pixel; the yardstick is input_norm in the same run.
step    the graph-replayed ResNet-18 step at B = 1024 with shuffle + crop-flip on against off,
        alternating three times each; the question is whether the difference lies within the off
        runs' min-max spread.

mix     input_mix_kernel (mixup, CutMix, either; shuffle + crop-flip on) against input_aug with both
        parts on and input_norm, and softmax_ce_soft (smoothing alone, with mixup rows) against
        softmax_ce at B = 1024, ten classes: the same interleaved rounds.  The old kernels are
        unchanged code in the same library, so they are the baseline.
mix_step  the graph-replayed step with each of label_smoothing, mixup_alpha, cutmix_alpha on, and all
        three on top of shuffle + crop-flip, against all off: alternating, three runs each.

Each prints one JSON line and writes it to <out>/aug_probe_<what>.json.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, HW, N = 1024, 32, 16384
VARIANTS = (("input_norm", None), ("aug_off", dict(shuffle=False, augment="none")), ("aug_shuffle", dict(shuffle=True, augment="none")),
            ("aug_crop_flip", dict(shuffle=False, augment="crop-flip")),
            ("aug_both", dict(shuffle=True, augment="crop-flip")))


def _shard(dev):
    from serverless_learn_amd.data.device_synth import synth_on_device

    x, y = synth_on_device("cifar", N, seed=0, device=dev)
    return x.view(N, HW, HW, 3), y


def _timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n  # ms per call


def kernel(args) -> dict:
    from serverless_learn_amd.models.resnet import CIFAR_MEAN, CIFAR_STD
    from serverless_learn_amd.ops import cnn as K

    dev = torch.device("cuda:0")
    x, y = _shard(dev)
    out = torch.empty(B, HW, HW, 8, dtype=torch.bfloat16, device=dev)
    lab = torch.empty(B, dtype=torch.uint8, device=dev)
    params = torch.empty(B, 4, dtype=torch.int32, device=dev)
    cursor = torch.zeros(1, dtype=torch.int32, device=dev)

    def launcher(kw):
        if kw is None:
            return lambda: K.input_norm(x, y, cursor, B, out, lab, CIFAR_MEAN, CIFAR_STD)
        return lambda: K.input_aug(x, y, cursor, B, out, lab, params, CIFAR_MEAN, CIFAR_STD, seed=0, pad=4, **kw)

    fns = {name: launcher(kw) for name, kw in VARIANTS}
    for fn in fns.values():
        _timed(fn, 20)
    us = {name: [] for name in fns}
    for r in range(args.rounds):
        cursor.fill_(5 * r + 1)  # another batch, epoch and set of draws every round
        for name, fn in fns.items():
            us[name].append(1e3 * _timed(fn, args.launches))
    nbytes = B * HW * HW * (3 + 16)
    res = {"what": "kernel", "batch": B, "hw": HW, "records": N, "launches": args.launches, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0)}
    for name, v in us.items():
        med = statistics.median(v)
        res[name] = {"us_median": round(med, 3), "us_min": round(min(v), 3), "us_max": round(max(v), 3),
                     "gbps": round(nbytes / (med * 1e-6) / 1e9, 1), "us_rounds": [round(t, 3) for t in v]}
    return res


def step(args) -> dict:
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    dev = torch.device("cuda:0")
    x, y = _shard(dev)
    trainers = {}
    for name, kw in (("off", {}), ("on", dict(shuffle=True, augment="crop-flip"))):
        tr = FusedResNetTrainer(batch=B, device=dev, seed=0, **kw)
        tr.load_shard(x, y)
        tr.step()
        tr.capture(warmup=1)
        _timed(tr.step, 10)
        trainers[name] = tr
    ms = {name: [] for name in trainers}
    for _ in range(3):
        for name, tr in trainers.items():
            ms[name].append(_timed(tr.step, args.steps))
    res = {"what": "step", "batch": B, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    for name, v in ms.items():
        res[name] = {"ms_runs": [round(t, 4) for t in v], "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                     "ms_median": round(statistics.median(v), 4), "loss": round(trainers[name].stats().loss, 4)}
    diff = res["on"]["ms_median"] - res["off"]["ms_median"]
    res["on_minus_off_ms"] = round(diff, 4)
    res["off_spread_ms"] = round(res["off"]["ms_max"] - res["off"]["ms_min"], 4)
    res["within_off_spread"] = abs(diff) <= res["off_spread_ms"]
    return res


MIX_VARIANTS = (("mix_mixup", dict(mixup=True)), ("mix_cutmix", dict(cutmix=True)),
                ("mix_either", dict(mixup=True, cutmix=True)))


def mix(args) -> dict:
    from serverless_learn_amd.data import augment as A
    from serverless_learn_amd.models.resnet import CIFAR_MEAN, CIFAR_STD
    from serverless_learn_amd.ops import cnn as K

    dev = torch.device("cuda:0")
    x, y = _shard(dev)
    out = torch.empty(B, HW, HW, 8, dtype=torch.bfloat16, device=dev)
    lab = torch.empty(B, dtype=torch.uint8, device=dev)
    params = torch.empty(B, 4, dtype=torch.int32, device=dev)
    mix_out = torch.zeros(B, 8, dtype=torch.int32, device=dev)
    table = torch.from_numpy(A.mix_tables(0.4, 1.0)).to(dev)
    cursor = torch.zeros(1, dtype=torch.int32, device=dev)
    both = dict(shuffle=True, augment="crop-flip")
    fns = {"input_norm": lambda: K.input_norm(x, y, cursor, B, out, lab, CIFAR_MEAN, CIFAR_STD),
           "aug_both": lambda: K.input_aug(x, y, cursor, B, out, lab, params, CIFAR_MEAN, CIFAR_STD, seed=0, pad=4,
                                           **both)}
    for name, kw in MIX_VARIANTS:
        fns[name] = (lambda kw: lambda: K.input_mix(x, y, cursor, B, out, lab, params, mix_out, table, CIFAR_MEAN,
                                                    CIFAR_STD, seed=0, pad=4, **both, **kw))(kw)
    z = torch.randn(B, 10, device=dev) * 3
    loss, corr = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    dz = torch.zeros(B, 16, dtype=torch.bfloat16, device=dev)
    db = torch.zeros(10, device=dev)
    fns["softmax_ce"] = lambda: K.softmax_ce(z, lab, loss, corr, dz, db, 1.0 / B)
    fns["soft_smoothing"] = lambda: K.softmax_ce_soft(z, lab, loss, corr, dz, db, 1.0 / B, mix=None, eps=0.1)
    fns["soft_mix"] = lambda: K.softmax_ce_soft(z, lab, loss, corr, dz, db, 1.0 / B, mix=mix_out, eps=0.1)
    fns["mix_mixup"]()  # mix_out rows for soft_mix
    for fn in fns.values():
        _timed(fn, 20)
    us = {name: [] for name in fns}
    for r in range(args.rounds):
        cursor.fill_(5 * r + 1)
        for name, fn in fns.items():
            us[name].append(1e3 * _timed(fn, args.launches))
    res = {"what": "mix", "batch": B, "hw": HW, "records": N, "launches": args.launches, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0)}
    for name, v in us.items():
        res[name] = {"us_median": round(statistics.median(v), 3), "us_min": round(min(v), 3),
                     "us_max": round(max(v), 3), "us_rounds": [round(t, 3) for t in v]}
    return res


def mix_step(args) -> dict:
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    dev = torch.device("cuda:0")
    x, y = _shard(dev)
    cases = (("off", {}), ("smoothing", dict(label_smoothing=0.1)), ("mixup", dict(mixup_alpha=0.4)),
             ("cutmix", dict(cutmix_alpha=1.0)),
             ("all", dict(label_smoothing=0.1, mixup_alpha=0.4, cutmix_alpha=1.0, shuffle=True, augment="crop-flip")))
    trainers = {}
    for name, kw in cases:
        tr = FusedResNetTrainer(batch=B, device=dev, seed=0, **kw)
        tr.load_shard(x, y)
        tr.step()
        tr.capture(warmup=1)
        _timed(tr.step, 10)
        trainers[name] = tr
    ms = {name: [] for name in trainers}
    for _ in range(3):
        for name, tr in trainers.items():
            ms[name].append(_timed(tr.step, args.steps))
    res = {"what": "mix_step", "batch": B, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    for name, v in ms.items():
        res[name] = {"ms_runs": [round(t, 4) for t in v], "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                     "ms_median": round(statistics.median(v), 4), "loss": round(trainers[name].stats().loss, 4)}
    res["off_spread_ms"] = round(res["off"]["ms_max"] - res["off"]["ms_min"], 4)
    for name in ms:
        if name != "off":
            res[name]["minus_off_ms"] = round(res[name]["ms_median"] - res["off"]["ms_median"], 4)
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "step", "mix", "mix_step"])
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=60)
    args = ap.parse_args(argv)
    res = {"kernel": kernel, "step": step, "mix": mix, "mix_step": mix_step}[args.what](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"aug_probe_{args.what}.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
