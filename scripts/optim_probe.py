#!/usr/bin/env python3
"""In-process interleaved timing of the optimizer rules (cdna_hip_programming.md rule 24).

bench.py measures the default rule only (momentum SGD at a fixed lr).  Here one trainer per
rule is built on the same shard, each captures its step graph once, and the arms alternate
over R rounds of K timed steps between device events around synchronised replays; medians in
us per step are printed as JSON.

Arms: MLP (default B = 65,536): sgd (the default launches), sgd+cosine, adamw+cosine.
      ResNet-18 (--model resnet18, default B = 1,024): sgd, adamw.
Usage: python scripts/optim_probe.py [--model mlp|resnet18] [--batch B] [--rounds 6] [--steps 50]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="mlp", choices=["mlp", "resnet18"])
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--steps", type=int, default=50)
a = ap.parse_args()
horizon = 4 * a.rounds * a.steps  # the schedules keep moving over the whole probe
cosine = dict(lr_schedule="cosine", lr_warmup_steps=100, lr_decay_steps=horizon)
if a.model == "mlp":
    from serverless_learn_amd.data.synthetic import make_mnist_like
    from serverless_learn_amd.models.mlp import FusedMLPTrainer

    B = a.batch or 65536
    x, y = make_mnist_like(4 * B, seed=0)  # 4 batches: X streams from HBM, as in bench.py
    arms = {"sgd": {}, "sgd+cosine": cosine, "adamw+cosine": dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2, **cosine)}
    make = lambda kw: FusedMLPTrainer(batch=B, device="cuda:0", **kw)  # noqa: E731
else:
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    B = a.batch or 1024
    x, y = make_cifar_like(2 * B, seed=0)
    arms = {"sgd": {}, "adamw": dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2)}
    make = lambda kw: FusedResNetTrainer(batch=B, device="cuda:0", **kw)  # noqa: E731
xs, ys = torch.from_numpy(x), torch.from_numpy(y)
trs = {}
for name, kw in arms.items():
    trs[name] = tr = make(kw)
    tr.load_shard(xs, ys)
    if a.model == "mlp":
        tr.capture(warmup=2, unroll=a.steps)
    else:
        tr.capture(warmup=2)


def run(tr, n):
    if a.model == "mlp":
        tr.steps(n)
    else:
        for _ in range(n):
            tr.step()


t = {name: [] for name in arms}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for r in range(a.rounds):
    for name, tr in trs.items():
        run(tr, a.steps)  # warm
        torch.cuda.synchronize()
        e0.record()
        run(tr, a.steps)
        e1.record()
        torch.cuda.synchronize()
        t[name].append(e0.elapsed_time(e1) / a.steps * 1e3)  # us per step
res = {"model": a.model, "batch": B, "rounds": a.rounds, "steps": a.steps,
       "arms": {name: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                       "all": [round(u, 2) for u in v]} for name, v in t.items()}}
base = res["arms"]["sgd"]["median_us"]
for name in arms:
    res["arms"][name]["over_sgd"] = round(res["arms"][name]["median_us"] / base, 4)
print(json.dumps(res, indent=1))
for tr in trs.values():
    tr.drop_graphs()
