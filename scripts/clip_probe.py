#!/usr/bin/env python3
"""In-process interleaved timing of gradient clipping (a sibling of scripts/optim_probe.py).

One trainer per arm on the same shard, each captures its step graph once, and the arms
alternate over R rounds of K timed steps between device events around synchronised replays;
medians in us per step are printed as JSON.

Arms, MLP (default B = 65,536):
  fused          the default step: slab reduce + update in one launch            (a)
  reduce_update  identity all-reduce hook: reduce launch, then update launch     (b)
  clip           clip_grad_norm below the norm: (b) + the two clip launches, scaling
  clip_inf       clip_grad_norm = inf: (b) + the two clip launches, the walk skipped
Arms, ResNet-18 (--model resnet18, default B = 1,024): sgd ((a) and (b) are one step there),
clip, clip_inf.
Usage: python scripts/clip_probe.py [--model mlp|resnet18] [--batch B] [--rounds 6] [--steps 50]
"""
import argparse
import json
import math
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
ap.add_argument("--max-norm", type=float, default=0.01, help="the clip arm's max_norm (below every step's norm)")
a = ap.parse_args()
clip, clip_inf = dict(clip_grad_norm=a.max_norm), dict(clip_grad_norm=math.inf)
if a.model == "mlp":
    from serverless_learn_amd.data.synthetic import make_mnist_like
    from serverless_learn_amd.models.mlp import FusedMLPTrainer

    B = a.batch or 65536
    x, y = make_mnist_like(4 * B, seed=0)  # 4 batches: X streams from HBM, as in bench.py
    arms = {"fused": {}, "reduce_update": {}, "clip": clip, "clip_inf": clip_inf}
    make = lambda kw: FusedMLPTrainer(batch=B, device="cuda:0", **kw)  # noqa: E731
    base = "fused"
else:
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    B = a.batch or 1024
    x, y = make_cifar_like(2 * B, seed=0)
    arms = {"sgd": {}, "clip": clip, "clip_inf": clip_inf}
    make = lambda kw: FusedResNetTrainer(batch=B, device="cuda:0", **kw)  # noqa: E731
    base = "sgd"
xs, ys = torch.from_numpy(x), torch.from_numpy(y)
trs = {}
for name, kw in arms.items():
    trs[name] = tr = make(kw)
    tr.load_shard(xs, ys)
    if name == "reduce_update":
        tr.allreduce = lambda g: None  # identity: the step takes the reduce -> update launches
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
norms = {name: [] for name in arms}
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
        norms[name].append(tr.grad_norm())
res = {"model": a.model, "batch": B, "rounds": a.rounds, "steps": a.steps, "max_norm": a.max_norm,
       "arms": {name: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                       "all": [round(u, 2) for u in v]} for name, v in t.items()}}
for name in arms:
    res["arms"][name]["over_" + base] = round(res["arms"][name]["median_us"] / res["arms"][base]["median_us"], 4)
    if norms[name][0] is not None:
        res["arms"][name]["grad_norm"] = [round(v, 5) for v in norms[name]]
print(json.dumps(res, indent=1))
for tr in trs.values():
    tr.drop_graphs()
