#!/usr/bin/env python3
"""In-process interleaved timing of the decay groups (cdna_hip_programming.md rule 24): ungrouped
against grouped, same rule, arms alternating over R rounds between device events; medians in us.

  --what kernel   the update launch alone, replayed from a graph of K launches: the flat kernel at
                  ResNet-18's parameter count (sl_adamw_flat / sl_sgd_flat_lr against their _groups
                  siblings, with the bf16 shadow) and the MLP's update from a gradient at its
                  269,322 parameters (sl_mlp_opt against sl_mlp_opt_groups)
  --what mlp      the captured MLP step (default B = 65,536), AdamW and scheduled SGD
  --what resnet18 the captured ResNet-18 step (default B = 1,024), AdamW and scheduled SGD
Usage: python scripts/groups_probe.py --what kernel|mlp|resnet18 [--batch B] [--rounds 6] [--steps 50]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--what", default="kernel", choices=["kernel", "mlp", "resnet18"])
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--steps", type=int, default=50)
a = ap.parse_args()
DEV = "cuda:0"
horizon = 4 * a.rounds * a.steps
RULES = {"adamw": dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2, lr_schedule="cosine", lr_warmup_steps=100,
                       lr_decay_steps=horizon),
         "sgd": dict(lr=0.05, momentum=0.9, weight_decay=5e-4, lr_schedule="cosine", lr_warmup_steps=100,
                     lr_decay_steps=horizon)}
GROUPS = dict(norm_weight_decay=0.0, bias_weight_decay=0.0)
arms = {}  # name -> callable(n): n steps / launches

if a.what == "kernel":
    from serverless_learn_amd.models.mlp import FusedMLPTrainer
    from serverless_learn_amd.models.resnet import CPUResNetTrainer
    from serverless_learn_amd.ops import optim as O

    ref = CPUResNetTrainer(batch=2, **GROUPS)
    n = ref.spec.n_flat
    cls = ref.decay_cls.to(DEV)
    w, g, m, v = (torch.randn(n, device=DEV) * 0.05 for _ in range(4))
    v.abs_()
    sh = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for rule, kw in RULES.items():
        spec_u, spec_g = O.OptSpec(**kw), O.OptSpec(**kw, **GROUPS)
        tab = torch.from_numpy(spec_u.lr_table()).to(DEV)
        if rule == "adamw":
            launch = {"": lambda s=spec_u, t=tab: O.adamw_flat(w, g, m, v, step, s, t, shadow=sh),
                      "+groups": lambda s=spec_g, t=tab: O.adamw_flat_groups(w, g, m, v, step, s, cls, t, shadow=sh)}
        else:
            launch = {"": lambda s=spec_u, t=tab: O.sgd_flat_lr(w, g, m, step, t, s.momentum, s.weight_decay, shadow=sh),
                      "+groups": lambda s=spec_g, t=tab: O.sgd_flat_lr_groups(w, g, m, step, t, cls, s.decays(),
                                                                              momentum=s.momentum, shadow=sh)}
        for sfx, fn in launch.items():
            arms[f"flat {rule}{sfx} n={n}"] = fn
    keep = []
    for rule, kw in RULES.items():
        for sfx, grp in (("", {}), ("+groups", dict(bias_weight_decay=0.0))):
            tr = FusedMLPTrainer(batch=64, device=DEV, **kw, **grp)
            keep.append(tr)
            arms[f"mlp update {rule}{sfx}"] = tr._launches()["update"]
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in arms.items():  # K launches per replay: the launch itself, not the host's call
        fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            for _ in range(a.steps):
                fn()
        graphs[name] = gr
    run = {name: (lambda n_, gr=gr: gr.replay()) for name, gr in graphs.items()}
else:
    if a.what == "mlp":
        from serverless_learn_amd.data.synthetic import make_mnist_like
        from serverless_learn_amd.models.mlp import FusedMLPTrainer

        B = a.batch or 65536
        x, y = make_mnist_like(4 * B, seed=0)
        make = lambda kw: FusedMLPTrainer(batch=B, device=DEV, **kw)  # noqa: E731
        grp = dict(bias_weight_decay=0.0)
    else:
        from serverless_learn_amd.data.synthetic import make_cifar_like
        from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

        B = a.batch or 1024
        x, y = make_cifar_like(2 * B, seed=0)
        make = lambda kw: FusedResNetTrainer(batch=B, device=DEV, **kw)  # noqa: E731
        grp = GROUPS
    xs, ys = torch.from_numpy(x), torch.from_numpy(y)
    trs = {}
    for rule, kw in RULES.items():
        for sfx, extra in (("", {}), ("+groups", grp)):
            trs[f"{a.what} B={B} {rule}{sfx}"] = tr = make(dict(kw, **extra))
            tr.load_shard(xs, ys)
            tr.capture(warmup=2, **(dict(unroll=a.steps) if a.what == "mlp" else {}))

    def stepper(tr):
        if a.what == "mlp":
            return tr.steps
        return lambda n_: [tr.step() for _ in range(n_)]

    run = {name: stepper(tr) for name, tr in trs.items()}

t = {name: [] for name in run}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for r in range(a.rounds):
    for name, fn in run.items():
        fn(a.steps)  # warm
        torch.cuda.synchronize()
        e0.record()
        fn(a.steps)
        e1.record()
        torch.cuda.synchronize()
        t[name].append(e0.elapsed_time(e1) / a.steps * 1e3)  # us per step / launch
res = {"what": a.what, "rounds": a.rounds, "steps": a.steps,
       "arms": {name: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                       "all": [round(u, 2) for u in v]} for name, v in t.items()}}
for name in run:
    if name.endswith("+groups") or "+groups " in name:
        base = res["arms"][name.replace("+groups", "")]["median_us"]
        res["arms"][name]["over_ungrouped"] = round(res["arms"][name]["median_us"] / base, 4)
print(json.dumps(res, indent=1))
if a.what != "kernel":
    for tr in trs.values():
        tr.drop_graphs()
