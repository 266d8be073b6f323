#!/usr/bin/env python3
"""Decay groups in the deterministic kernel build (SL_DETERMINISTIC=1; a process loads one kernel
library, so the tests run this in a child process).  Everything is compared bit for bit:

* the flat kernels' grouped launches against the ungrouped ones, per class
  (serverless_learn_amd/utils/decay_exact.py);
* the ResNet engine, one step from the same seed and shard: a grouped trainer (weight 0.5, norm
  0.25, bias 0) has the class-c elements of params / mom / v of the ungrouped trainer run with
  class c's decay, under AdamW and under scheduled SGD;
* the ResNet engine under AdamW with all three decays equal: n steps equal the ungrouped
  trainer's, and n steps replayed from a captured graph equal n eager steps.

Prints one JSON line.  Usage: SL_DETERMINISTIC=1 python scripts/decay_groups_det.py [batch] [n]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from serverless_learn_amd.data.synthetic import make_cifar_like
from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer
from serverless_learn_amd.ops import cnn as K
from serverless_learn_amd.ops import optim as O
from serverless_learn_amd.utils.decay_exact import flat_failures, select_by_class

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
n = int(sys.argv[2]) if len(sys.argv) > 2 else 3
DEV = "cuda:0"
x, y = make_cifar_like(2 * batch, seed=5)
x, y = torch.from_numpy(x), torch.from_numpy(y)
RULES = {"adamw": dict(optimizer="adamw", lr=1e-3, lr_warmup_steps=3),
         "sgd": dict(lr=0.05, momentum=0.9, lr_schedule="cosine", lr_warmup_steps=2, lr_decay_steps=8)}
W, NORM, BIAS = 0.5, 0.25, 0.0


def trainer(**kw):
    t = FusedResNetTrainer(batch=batch, device=DEV, seed=2, **kw)
    t.load_shard(x, y)
    return t


def state(t):
    torch.cuda.synchronize()
    return {k: getattr(t, k).clone() for k in ("params", "mom", "v") if getattr(t, k) is not None}


def same(a: dict, b: dict) -> bool:
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


out = {"deterministic_build": K.deterministic(), "batch": batch, "n": n, "flat_failures": flat_failures(DEV)}

# one step, three classes
for rule, kw in RULES.items():
    g = trainer(weight_decay=W, norm_weight_decay=NORM, bias_weight_decay=BIAS, **kw)
    cls = g.decay_cls.cpu().numpy()
    g.step()
    got = state(g)
    refs = []
    for wd in (W, NORM, BIAS):
        u = trainer(weight_decay=wd, **kw)
        u.step()
        refs.append(state(u))
        del u
    bad = [k for k, t in got.items()
           if not torch.equal(t, select_by_class(cls, t.numel(), [r[k] for r in refs]))]
    counts = O.decay_class_counts(cls, g.n_params)
    out[f"compose_{rule}"] = {"differ": bad, "tensors": sorted(got), "class_elements": counts,
                              "refs_distinct": not same(refs[0], refs[1]) and not same(refs[1], refs[2]),
                              "shadow_ok": bool(torch.equal(g.shadow, g.params.to(torch.bfloat16)))}
    del g, refs

# equal decays: grouped == ungrouped, graph == eager
kw = dict(weight_decay=1e-2, **RULES["adamw"])
grp = dict(norm_weight_decay=1e-2, bias_weight_decay=1e-2)
a, b, u = trainer(**kw, **grp), trainer(**kw, **grp), trainer(**kw)
for t in (a, b, u):
    t.step()  # eager: sizes the split-K workspace before the capture
a.capture(warmup=0)
for _ in range(n):
    for t in (a, b, u):
        t.step()
sa, sb, su = state(a), state(b), state(u)
out["equal_decays"] = {"graph_equals_eager": same(sa, sb), "grouped_equals_ungrouped": same(sb, su),
                       "opt_step": [int(t.opt_step.item()) for t in (a, b, u)],
                       "finite": bool(torch.isfinite(sa["params"]).all())}
out["ungrouped_has_map"] = hasattr(u, "decay_cls")
print(json.dumps(out))
a.drop_graphs()
