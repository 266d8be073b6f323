#!/usr/bin/env python3
"""The weight EMA in the ResNet engine against its definition, in the deterministic kernel build
(SL_DETERMINISTIC=1: a process loads one kernel library, so tests/test_ema_gpu.py runs this as a
child).  ResNet-18, CIFAR stem, batch 32, ema_decay 0.5 (a 9-entry warm-up table).  Prints one JSON line.

eager     6 eager steps with a get_flat() snapshot after each: ema_flat() must equal the recurrence
          e <- e + omd_t * (w - e) over the snapshots (torch fp32 on the host) bit for bit, and
          parameters, momentum, bf16 shadow and running statistics must equal an EMA-off twin's.
graph     the same recurrence on a second trainer whose steps come from a captured graph replayed one
          at a time (after capture()'s two eager warm-up steps); it ends bit-identical to `eager`.
evaluate  evaluate(ema=True) against a second trainer after set_flat(ema_flat()) with the running
          statistics copied; parameters, shadow, transposed weights, running statistics, momentum,
          the EMA and the counters are bit-identical before and after, and the next step still equals
          the twin's.
resume    three steps (AdamW), save through the checkpoint byte format, restore into a fresh trainer
          with another seed, three more steps in both: bit-identical, the EMA included.  A file
          without the keys starts the EMA from the loaded weights at step 0.

Usage: SL_DETERMINISTIC=1 python scripts/ema_resnet_det.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from serverless_learn_amd.ckpt import format as ckfmt
from serverless_learn_amd.data.synthetic import make_cifar_like
from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer
from serverless_learn_amd.ops import cnn as K
from serverless_learn_amd.ops import optim as O

B, D, STEPS, DEV = 32, 0.5, 6, "cuda:0"
x, y = make_cifar_like(6 * B, seed=5)
x, y = torch.from_numpy(x), torch.from_numpy(y)
TAB = torch.from_numpy(O.ema_table(D, True))


def trainer(seed=2, **kw):
    tr = FusedResNetTrainer(batch=B, device=DEV, seed=seed, **kw)
    tr.load_shard(x, y)
    return tr


def same_stats(a, b) -> bool:
    return all(torch.equal(rm, b.running_stats()[name][0]) and torch.equal(rv, b.running_stats()[name][1])
               for name, (rm, rv) in a.running_stats().items())


def follow(tr, steps: int, e: torch.Tensor, t0: int) -> tuple:
    """``steps`` steps of ``tr``; after each, ema_flat() against the recurrence over the snapshots."""
    ok = []
    for t in range(t0, t0 + steps):
        tr.step()
        w = tr.get_flat().cpu()
        e = e + TAB[min(t, TAB.numel() - 1)] * (w - e)
        ok.append(bool(torch.equal(tr.ema_flat().cpu(), e)) and int(tr.ema_step.item()) == t + 1)
    return ok, e


def training_state(tr) -> dict:
    d = {"params": tr.params, "shadow": tr.shadow, "mom": tr.mom, "ema": tr.ema, "ema_step": tr.ema_step,
         "ema_ticket": tr.ema_ticket, "cursor": tr.cursor, "fc_wt": tr.fc_wt}
    d.update({f"wt/{name}": c.wt for name, c in tr.conv.items()})
    for name, (rm, rv) in tr.running_stats().items():
        d[f"bn/{name}/mean"], d[f"bn/{name}/var"] = rm, rv
    return {k: v.clone() for k, v in d.items() if v is not None}


out = {"deterministic_build": K.deterministic()}

# ---- eager, against the recurrence and the EMA-off twin ----
tr, twin = trainer(ema_decay=D), trainer()
res = {"starts_at_params": bool(torch.equal(tr.ema_flat(), tr.get_flat())), "table": int(tr.ema_tab.numel()),
       "twin_has_no_ema": twin.ema is None and twin.ema_step is None and twin.ema_ticket is None}
ok, e_eager = follow(tr, STEPS, tr.get_flat().cpu(), 0)
for _ in range(STEPS):
    twin.step()
torch.cuda.synchronize()
res.update(recurrence=ok, ema_step=int(tr.ema_step.item()), ticket=int(tr.ema_ticket.item()),
           ema_differs_from_params=not bool(torch.equal(tr.ema, tr.params)),
           params_identical=bool(torch.equal(tr.params, twin.params)), mom_identical=bool(torch.equal(tr.mom, twin.mom)),
           shadow_identical=bool(torch.equal(tr.shadow, twin.shadow)), running_stats_identical=same_stats(tr, twin),
           cursor=[int(tr.cursor.item()), int(twin.cursor.item())], finite=bool(torch.isfinite(tr.ema).all()),
           buffers_extra=len(tr.buffers()) - len(twin.buffers()),
           buffers_carry_ema=tr.buffers()[-2] is tr.ema and tr.buffers()[-1] is tr.ema_step,
           state_keys_extra=sorted(set(tr.state_extra()) - set(twin.state_extra())),
           twin_state_keys_as_before=not any(k.startswith("ema") for k in twin.state_extra()))
out["eager"] = res

# ---- from a captured graph, replayed step by step ----
g = trainer(ema_decay=D)
e0 = g.get_flat().cpu()
warm = 2
g.capture(warmup=warm)  # two eager steps, then the capture
torch.cuda.synchronize()
# capture() took the warm-up steps without a snapshot: a third trainer takes the same two (same seed, same
# shard, deterministic build) under the recurrence, and the graph trainer must stand where it stands
chk = trainer(ema_decay=D)
okw, e_w = follow(chk, warm, e0, 0)
pre = bool(torch.equal(g.ema_flat().cpu(), e_w)) and bool(torch.equal(g.params, chk.params))
ok, e_graph = follow(g, STEPS - warm, e_w, warm)
torch.cuda.synchronize()
out["graph"] = {"captured": g.graph is not None, "after_warmup_identical": pre and all(okw), "recurrence": ok,
                "ema_step": int(g.ema_step.item()), "ticket": int(g.ema_ticket.item()),
                "ema_identical_to_eager": bool(torch.equal(g.ema, tr.ema)),
                "params_identical_to_eager": bool(torch.equal(g.params, tr.params)),
                "mom_identical_to_eager": bool(torch.equal(g.mom, tr.mom)),
                "running_stats_identical": same_stats(g, tr)}
del chk

# ---- evaluate(ema=True) ----
before = training_state(tr)
ptrs = {k: getattr(tr, k).data_ptr() for k in ("params", "shadow", "ema", "mom")}
own, avg = tr.evaluate(x, y), tr.evaluate(x, y, ema=True)
torch.cuda.synchronize()
after = training_state(tr)
second = trainer(seed=9)
second.set_flat(tr.ema_flat())
for name, (rm, rv) in tr.running_stats().items():
    second.running_stats()[name][0].copy_(rm)
    second.running_stats()[name][1].copy_(rv)
want = second.evaluate(x, y)
res = {"equals_second_trainer": (avg.loss, avg.accuracy, avg.n) == (want.loss, want.accuracy, want.n),
       "differs_from_params": (avg.loss, avg.accuracy) != (own.loss, own.accuracy), "n": avg.n,
       "state_identical": sorted(k for k in before if not torch.equal(before[k], after[k])) == [],
       "state_tensors": len(before),
       "no_tensor_moved": all(getattr(tr, k).data_ptr() == p for k, p in ptrs.items())}
try:
    twin.evaluate(x, y, ema=True)
    res["raises_without_ema"] = False
except ValueError:
    res["raises_without_ema"] = True
# the graph trainer evaluates too, then replays: equal to the eager pair's next step
g.evaluate(x, y, ema=True)
for t in (tr, twin, g):
    t.step()
torch.cuda.synchronize()
res["next_step_equals_twin"] = bool(torch.equal(tr.params, twin.params)) and same_stats(tr, twin)
res["next_replay_equals_eager"] = (bool(torch.equal(g.params, tr.params)) and bool(torch.equal(g.ema, tr.ema))
                                   and g.graph is not None)
out["evaluate"] = res
del second, g

# ---- resume ----
kw = dict(ema_decay=D, optimizer="adamw", lr=1e-3, weight_decay=1e-2)
a = trainer(**kw)
for _ in range(3):
    a.step()
n = a.n_params
buf = ckfmt.encode(a.get_flat().cpu().numpy(), {"model": a.model_name, "step": 3}, a.mom[:n].cpu().numpy(),
                   a.state_extra())
meta, params, mom, extra = ckfmt.decode_full(buf)
b = trainer(seed=7, **kw)
differs_before = not bool(torch.equal(a.ema, b.ema))
b.set_flat(torch.from_numpy(params))
b.mom[:n].copy_(torch.from_numpy(mom))
b.load_state_extra(extra)
loaded = bool(torch.equal(a.ema, b.ema)) and int(b.ema_step.item()) == 3
for _ in range(3):
    a.step()
    b.step()
torch.cuda.synchronize()
res = {"fresh_trainer_differs": differs_before, "loaded_identical": loaded,
       "ema_identical": bool(torch.equal(a.ema, b.ema)), "params_identical": bool(torch.equal(a.params, b.params)),
       "mom_identical": bool(torch.equal(a.mom, b.mom)), "v_identical": bool(torch.equal(a.v, b.v)),
       "running_stats_identical": same_stats(a, b), "ema_step": [int(a.ema_step.item()), int(b.ema_step.item())],
       "ckpt_ema_step": int(extra["ema_step"][0]), "ckpt_ema_size": int(extra["ema"].size), "n_params": n}
b.load_state_extra({k: v for k, v in extra.items() if k not in ("ema", "ema_step")})
res["without_keys_from_weights"] = bool(torch.equal(b.ema, b.params)) and int(b.ema_step.item()) == 0
out["resume"] = res
print(json.dumps(out))
