#!/usr/bin/env python
"""What gradient accumulation costs (profiles/r15_accum).

Three measurements, each a process of its own so that each runs under its own time limit:

    timeout -k 10 300 python scripts/accum_probe.py kernel --out profiles/r15_accum && \\
    timeout -k 10 300 python scripts/accum_probe.py mlp --out profiles/r15_accum && \\
    timeout -k 10 600 python scripts/accum_probe.py resnet --out profiles/r15_accum

kernel  accum_flat (store, add, add on views that start one element past a 16-byte boundary, add with
        only the source misaligned) against sgd_flat with momentum and the bf16 shadow, the update
        launch of the same vector, at the MLP's and the ResNet-18's parameter counts: device events
        around 200 launches of each, interleaved, several rounds.  Microseconds per launch and the
        GB/s implied by the bytes each moves (8 / 12 per element; sgd_flat 22).
mlp     the captured MLP step at B = 65536.  For K in (2, 4): a trainer with accum_steps = K, one
        graph replay per step, against K back-to-back steps of a trainer with accum_steps = 1
        captured with unroll = K (one replay per K steps: the same launches as before accumulation
        existed, so this is the parent's cost at the same batch).  `k1` takes the fused slab update;
        `k1_hook` has the identity exchange hook, so it takes the reduce -> update pair an
        accumulating step also takes and isolates the accumulate launches.  Alternating, three runs.
resnet  the same for the captured ResNet-18 step at B = 1024 (no hook variant: the engine has one
        update path).

Each prints one JSON line and writes it to <out>/accum_probe_<what>.json.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (2, 4)


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


def kernel(args) -> dict:
    from serverless_learn_amd.models.mlp import N_PARAMS
    from serverless_learn_amd.models.resnet import resnet18_spec
    from serverless_learn_amd.ops import optim as O

    dev = torch.device("cuda:0")
    res = {"what": "kernel", "launches": args.launches, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    for label, n in (("mlp", N_PARAMS), ("resnet18", resnet18_spec("cifar", 10, None).n_flat)):
        a, b = torch.randn(n + 8, device=dev), torch.randn(n + 8, device=dev)
        w, mom = torch.randn(n, device=dev) * 0.05, torch.zeros(n, device=dev)
        sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        fns = {"store": (8, lambda: O.accum_flat(a[:n], b[:n], False)),
               "add": (12, lambda: O.accum_flat(a[:n], b[:n], True)),
               "add_offset_1_1": (12, lambda: O.accum_flat(a[1:n + 1], b[1:n + 1], True)),
               "add_src_offset_2": (12, lambda: O.accum_flat(a[:n], b[2:n + 2], True)),
               "sgd_flat": (22, lambda: O.sgd_flat(w, b[:n], mom, 1e-3, 0.9, 1e-4, shadow=sh))}
        for _, fn in fns.values():
            _timed(fn, 20)
        us = {name: [] for name in fns}
        for _ in range(args.rounds):
            a.normal_()  # fresh values every round: the sums of 200 adds stay small
            for name, (_, fn) in fns.items():
                us[name].append(1e3 * _timed(fn, args.launches))
        res[label] = {"n": n}
        for name, v in us.items():
            med = statistics.median(v)
            res[label][name] = dict(_summary(v, "us", 3), gbps=round(fns[name][0] * n / (med * 1e-6) / 1e9, 1))
    return res


def _step_table(res: dict, ms: dict) -> dict:
    """ms[name]: per-run milliseconds for K micro-batches (name: k<K>, k1x<K>, k1_hookx<K>)."""
    for name, v in ms.items():
        res[name] = _summary(v)
    for k in KS:
        base = res[f"k1x{k}"]
        res[f"k{k}"]["minus_k1_ms"] = round(res[f"k{k}"]["ms_median"] - base["ms_median"], 4)
        res[f"k{k}"]["k1_spread_ms"] = round(base["ms_max"] - base["ms_min"], 4)
        res[f"k{k}"]["per_extra_micro_batch_us"] = round(1e3 * res[f"k{k}"]["minus_k1_ms"] / (k - 1), 2)
        if f"k1_hookx{k}" in res:
            res[f"k{k}"]["minus_k1_hook_ms"] = round(res[f"k{k}"]["ms_median"] - res[f"k1_hookx{k}"]["ms_median"], 4)
    return res


def mlp(args) -> dict:
    from serverless_learn_amd.data.device_synth import synth_on_device
    from serverless_learn_amd.models.mlp import FusedMLPTrainer

    dev = torch.device("cuda:0")
    B = 65536
    x, y = synth_on_device("mnist", 8 * B, seed=0, device=dev)
    runs = {}  # name -> callable running K micro-batches in one graph replay

    def make(k, unroll, hook=False):
        tr = FusedMLPTrainer(batch=B, device=dev, seed=0, accum_steps=k)
        tr.load_shard(x, y)
        if hook:
            tr.allreduce = lambda g: None
        tr.step()
        tr.capture(warmup=1, unroll=unroll)
        return tr

    keep = []
    for k in KS:
        acc, base, hook = make(k, 1), make(1, k), make(1, k, hook=True)
        keep += [acc, base, hook]
        runs[f"k{k}"] = acc.step
        runs[f"k1x{k}"] = (lambda t, k: lambda: t.steps(k))(base, k)
        runs[f"k1_hookx{k}"] = (lambda t, k: lambda: t.steps(k))(hook, k)
    for fn in runs.values():
        _timed(fn, 20)
    ms = {name: [] for name in runs}
    for _ in range(3):
        for name, fn in runs.items():
            ms[name].append(_timed(fn, args.steps))
    res = {"what": "mlp", "batch": B, "replays": args.steps, "device": torch.cuda.get_device_name(0)}
    res = _step_table(res, ms)
    res["loss"] = {name: round(t.stats().loss, 4) for name, t in zip(("k2", "k1x2", "k1_hookx2", "k4", "k1x4", "k1_hookx4"),
                                                                     keep)}
    return res


def resnet(args) -> dict:
    from serverless_learn_amd.data.device_synth import synth_on_device
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    dev = torch.device("cuda:0")
    B, N = 1024, 16384
    x, y = synth_on_device("cifar", N, seed=0, device=dev)
    x = x.view(N, 32, 32, 3)
    trainers = {}
    for k in (1,) + KS:
        tr = FusedResNetTrainer(batch=B, device=dev, seed=0, accum_steps=k)
        tr.load_shard(x, y)
        tr.step()
        tr.capture(warmup=1)
        trainers[k] = tr
    runs = {}
    for k in KS:
        runs[f"k{k}"] = trainers[k].step
        runs[f"k1x{k}"] = (lambda k: lambda: [trainers[1].step() for _ in range(k)])(k)
    for fn in runs.values():
        _timed(fn, 3)
    reps = max(1, args.steps // 10)
    ms = {name: [] for name in runs}
    for _ in range(3):
        for name, fn in runs.items():
            ms[name].append(_timed(fn, reps))
    res = {"what": "resnet", "batch": B, "replays": reps, "device": torch.cuda.get_device_name(0)}
    res = _step_table(res, ms)
    res["loss"] = {f"k{k}": round(t.stats().loss, 4) for k, t in trainers.items()}
    return res


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
        with open(os.path.join(args.out, f"accum_probe_{args.what}.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
