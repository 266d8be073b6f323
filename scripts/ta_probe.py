#!/usr/bin/env python
"""What TrivialAugment Wide costs in the ResNet engine's input pipeline (profiles/r25_ta).

Two measurements, each a process of its own so that each runs under its own time limit:

    timeout -k 10 300 python scripts/ta_probe.py kernel --out profiles/r25_ta && \\
    timeout -k 10 600 python scripts/ta_probe.py step --out profiles/r25_ta

kernel  input_ta_kernel at B = 1024 images of 32x32 out of a 16,384-record shard, shuffle + crop-flip
        on: with the operations drawn (what a trainer launches) and with each of the 14 pinned for
        the whole batch at bin 30, beside input_norm over the staging batch (the launch that follows
        it) and input_aug with both parts on (the launch the pair replaces).  Device events around
        200 launches of each, interleaved, several rounds with another cursor each.
step    the graph-replayed ResNet-18 step at B = 1024 with shuffle + crop-flip on, auto_augment off
        against trivial-wide, alternating three times each.

Each prints one JSON line and writes it to <out>/ta_probe_<what>.json.
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
PIPE = dict(shuffle=True, augment="crop-flip")


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
    from serverless_learn_amd.data import augment as A
    from serverless_learn_amd.models.resnet import CIFAR_MEAN, CIFAR_STD
    from serverless_learn_amd.ops import cnn as K

    dev = torch.device("cuda:0")
    x, y = _shard(dev)
    out = torch.empty(B, HW, HW, 8, dtype=torch.bfloat16, device=dev)
    ta_x = torch.empty(B, HW, HW, 3, dtype=torch.uint8, device=dev)
    lab, ta_lab = (torch.empty(B, dtype=torch.uint8, device=dev) for _ in range(2))
    params, ta_out = (torch.empty(B, 4, dtype=torch.int32, device=dev) for _ in range(2))
    table = torch.from_numpy(A.ta_table().copy()).to(dev)
    cursor = torch.zeros(1, dtype=torch.int32, device=dev)

    def ta(force):
        return lambda: K.input_ta(x, y, cursor, B, ta_x, ta_lab, params, ta_out, table, seed=0, pad=4, force=force,
                                  **PIPE)

    fns = {"input_norm_staged": lambda: K.input_norm(ta_x, ta_lab, cursor, B, out, lab, CIFAR_MEAN, CIFAR_STD),
           "aug_both": lambda: K.input_aug(x, y, cursor, B, out, lab, params, CIFAR_MEAN, CIFAR_STD, seed=0, pad=4,
                                           **PIPE),
           "ta_drawn": ta(-1)}
    for op, name in enumerate(A.TA_OPS):
        fns["ta_" + name] = ta(op | 30 << 8)
    for fn in fns.values():
        _timed(fn, 20)
    us = {name: [] for name in fns}
    for r in range(args.rounds):
        cursor.fill_(5 * r + 1)  # another batch, epoch and set of draws every round
        for name, fn in fns.items():
            us[name].append(1e3 * _timed(fn, args.launches))
    res = {"what": "kernel", "batch": B, "hw": HW, "records": N, "launches": args.launches, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0)}
    for name, v in us.items():
        res[name] = {"us_median": round(statistics.median(v), 3), "us_min": round(min(v), 3),
                     "us_max": round(max(v), 3)}
    return res


def step(args) -> dict:
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    dev = torch.device("cuda:0")
    x, y = _shard(dev)
    trainers = {}
    for name, kw in (("off", {}), ("on", dict(auto_augment="trivial-wide"))):
        tr = FusedResNetTrainer(batch=B, device=dev, seed=0, **PIPE, **kw)
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
    res["on_minus_off_ms"] = round(res["on"]["ms_median"] - res["off"]["ms_median"], 4)
    res["off_spread_ms"] = round(res["off"]["ms_max"] - res["off"]["ms_min"], 4)
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "step"])
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=60)
    args = ap.parse_args(argv)
    res = {"kernel": kernel, "step": step}[args.what](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"ta_probe_{args.what}.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
