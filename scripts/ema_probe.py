#!/usr/bin/env python
"""What the weight EMA costs (profiles/r16_ema).

Three measurements, each a process of its own so that each runs under its own time limit:

    timeout -k 10 300 python scripts/ema_probe.py kernel --out profiles/r16_ema && \\
    timeout -k 10 300 python scripts/ema_probe.py mlp --out profiles/r16_ema && \\
    timeout -k 10 600 python scripts/ema_probe.py resnet --out profiles/r16_ema

kernel  ema_flat against accum_flat's add (the same 12 bytes per element) and sgd_flat with momentum
        and the bf16 shadow (22 bytes), at the MLP's and the ResNet-18's parameter counts: device
        events around 200 launches of each, interleaved, several rounds.  Microseconds per launch and
        the GB/s implied.
mlp     the captured MLP step at B = 65536 with ema_decay = 0.999 against the same trainer with the EMA
        off, one graph replay per step, alternating, five runs.  `launches` lists what an eager step
        of each launches (the kernel library's entry points, in order): the EMA-off list is the
        parent's step.
resnet  the same for the captured ResNet-18 step at B = 1024.

Each prints one JSON line and writes it to <out>/ema_probe_<what>.json.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DECAY = 0.999


def _timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n  # ms per call


def _summary(v, unit="ms", digits=4):
    return {f"{unit}_runs": [round(t, digits) for t in v], f"{unit}_min": round(min(v), digits),
            f"{unit}_max": round(max(v), digits), f"{unit}_median": round(statistics.median(v), digits)}


def _entry_points(fn) -> list:
    """The kernel library's entry points ``fn`` calls, in order (cached launches and direct calls)."""
    from serverless_learn_amd.ops import _native as N

    names, call, launch = [], N.call, N.Launch.__call__

    def rec_call(name, *a):
        names.append(name)
        return call(name, *a)

    def rec_launch(self, stream=None):
        names.append(self.entry)
        return launch(self, stream)

    N.call, N.Launch.__call__ = rec_call, rec_launch
    try:
        fn()
    finally:
        N.call, N.Launch.__call__ = call, launch
    return names


def kernel(args) -> dict:
    from serverless_learn_amd.models.mlp import N_PARAMS
    from serverless_learn_amd.models.resnet import resnet18_spec
    from serverless_learn_amd.ops import optim as O

    dev = torch.device("cuda:0")
    res = {"what": "kernel", "launches": args.launches, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    tab = torch.from_numpy(O.ema_table(DECAY, True)).to(dev)
    for label, n in (("mlp", N_PARAMS), ("resnet18", resnet18_spec("cifar", 10, None).n_flat)):
        a, b = torch.randn(n, device=dev), torch.randn(n, device=dev)
        e, w, mom = torch.randn(n, device=dev), torch.randn(n, device=dev) * 0.05, torch.zeros(n, device=dev)
        sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        fns = {"ema_flat": (12, lambda: O.ema_flat(e, w, step, ticket, tab)),
               "accum_add": (12, lambda: O.accum_flat(a, b, True)),
               "sgd_flat": (22, lambda: O.sgd_flat(w, b, mom, 1e-3, 0.9, 1e-4, shadow=sh))}
        for _, fn in fns.values():
            _timed(fn, 20)
        us = {name: [] for name in fns}
        for _ in range(args.rounds):
            a.normal_()  # fresh values every round: the sums of 200 adds stay small
            for name, (_, fn) in fns.items():
                us[name].append(1e3 * _timed(fn, args.launches))
        res[label] = {"n": n, "ema_step": int(step.item()), "ticket": int(ticket.item())}
        for name, v in us.items():
            med = statistics.median(v)
            res[label][name] = dict(_summary(v, "us", 3), gbps=round(fns[name][0] * n / (med * 1e-6) / 1e9, 1))
    return res


def _on_off(res: dict, trainers: dict, reps: int, runs: int) -> dict:
    fns = {name: t.step for name, t in trainers.items()}
    for fn in fns.values():
        _timed(fn, max(3, reps // 10))
    ms = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():  # alternating
            ms[name].append(_timed(fn, reps))
    for name, v in ms.items():
        res[name] = _summary(v)
    res["on_minus_off_us"] = round(1e3 * (res["on"]["ms_median"] - res["off"]["ms_median"]), 2)
    res["on_over_off"] = round(res["on"]["ms_median"] / res["off"]["ms_median"], 5)
    res["off_spread_us"] = round(1e3 * (res["off"]["ms_max"] - res["off"]["ms_min"]), 2)
    res["loss"] = {name: round(t.stats().loss, 4) for name, t in trainers.items()}
    res["ema_step"] = int(trainers["on"].ema_step.item())
    return res


def mlp(args) -> dict:
    from serverless_learn_amd.data.device_synth import synth_on_device
    from serverless_learn_amd.models.mlp import FusedMLPTrainer

    dev = torch.device("cuda:0")
    B = 65536
    x, y = synth_on_device("mnist", 8 * B, seed=0, device=dev)
    trainers, launches = {}, {}
    for name, kw in (("off", {}), ("on", dict(ema_decay=DECAY))):
        tr = FusedMLPTrainer(batch=B, device=dev, seed=0, **kw)
        tr.load_shard(x, y)
        tr.step()
        launches[name] = _entry_points(tr._step_eager)
        tr.capture(warmup=1)
        trainers[name] = tr
    res = {"what": "mlp", "batch": B, "replays": args.steps, "ema_decay": DECAY, "launches": launches,
           "device": torch.cuda.get_device_name(0)}
    return _on_off(res, trainers, args.steps, 5)


def resnet(args) -> dict:
    from serverless_learn_amd.data.device_synth import synth_on_device
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    dev = torch.device("cuda:0")
    B, N = 1024, 16384
    x, y = synth_on_device("cifar", N, seed=0, device=dev)
    x = x.view(N, 32, 32, 3)
    trainers, launches = {}, {}
    for name, kw in (("off", {}), ("on", dict(ema_decay=DECAY))):
        tr = FusedResNetTrainer(batch=B, device=dev, seed=0, **kw)
        tr.load_shard(x, y)
        tr.step()
        names = _entry_points(tr._step_eager)
        launches[name] = {"count": len(names), "tail": names[-4:]}
        tr.capture(warmup=1)
        trainers[name] = tr
    reps = max(1, args.steps // 10)
    res = {"what": "resnet", "batch": B, "replays": reps, "ema_decay": DECAY, "launches": launches,
           "device": torch.cuda.get_device_name(0)}
    return _on_off(res, trainers, reps, 5)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "mlp", "resnet"])
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args(argv)
    res = {"kernel": kernel, "mlp": mlp, "resnet": resnet}[args.what](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"ema_probe_{args.what}.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
