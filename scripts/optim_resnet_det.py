#!/usr/bin/env python3
"""ResNet engine under AdamW + warm-up in the deterministic kernel build (SL_DETERMINISTIC=1):
after one eager step in each of two identical engines, n steps replayed from a captured graph
in one and n eager steps in the other must leave parameters and both moments bit-identical (the
optimizer step is read on the device, so the replays move through the warm-up).  Prints JSON.
Usage: SL_DETERMINISTIC=1 python scripts/optim_resnet_det.py [batch] [n]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from serverless_learn_amd.data.synthetic import make_cifar_like
from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer
from serverless_learn_amd.ops import cnn as K

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
n = int(sys.argv[2]) if len(sys.argv) > 2 else 3
x, y = make_cifar_like(2 * batch, seed=5)
x, y = torch.from_numpy(x), torch.from_numpy(y)
kw = dict(batch=batch, device="cuda:0", seed=2, optimizer="adamw", lr=1e-3, weight_decay=1e-2, lr_warmup_steps=3)
a, b = FusedResNetTrainer(**kw), FusedResNetTrainer(**kw)
for t in (a, b):
    t.load_shard(x, y)
    t.step()  # eager: sizes the split-K workspace before the capture
a.capture(warmup=0)
for _ in range(n):
    a.step()
    b.step()
torch.cuda.synchronize()
pa, pb = a.get_flat(), b.get_flat()
print(json.dumps({"deterministic_build": K.deterministic(), "batch": batch, "n": n,
                  "params_identical": bool(torch.equal(pa, pb)), "mom_identical": bool(torch.equal(a.mom, b.mom)),
                  "v_identical": bool(torch.equal(a.v, b.v)),
                  "opt_step": [int(a.opt_step.item()), int(b.opt_step.item())],
                  "param_max_diff": float((pa - pb).abs().max()), "finite": bool(torch.isfinite(pa).all())}))
a.drop_graphs()
