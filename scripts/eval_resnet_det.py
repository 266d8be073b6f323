#!/usr/bin/env python3
"""``evaluate_full`` in the ResNet engine against its definition, in the deterministic kernel build
(SL_DETERMINISTIC=1: a process loads one kernel library, and the comparison with a twin that never
evaluated needs bit-reproducible training steps; tests/test_eval_gpu.py runs this as a child).
ResNet-18, CIFAR stem, batch 32, a held-out set of N = 2 * 32 + 7 synthetic CIFAR records (three
batches, the last with 7 valid rows), ema_decay 0.5.  Prints one JSON line.

report    evaluate_full covers all N records and equals eval_reference applied to the logits and loss
          rows the engine itself produced for them (collected here by running forward_eval batch by
          batch over the same padded set); a second call gives the identical report; topk=1 counts
          what top1 counts; the cached padded copy is reused.
state     params, shadow, transposed weights, momentum, cursor, BN running statistics, ema / ema_step
          are bit-identical before and after, and no tensor moved.
graph     a step graph captured before the evaluation replays after it: bit-identical to a twin that
          never evaluated.
ema       evaluate_full(ema=True) equals evaluate_full on a second engine after set_flat(ema_flat())
          with the same running statistics, and differs from the live weights' report.
refusals  topk 0 and classes + 1, an empty set, ema=True without an EMA: ValueError.

Usage: SL_DETERMINISTIC=1 python scripts/eval_resnet_det.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from serverless_learn_amd.data.synthetic import make_cifar_like
from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer
from serverless_learn_amd.ops import cnn as K
from serverless_learn_amd.ops.evalmetrics import eval_reference

B, D, DEV, NCLS = 32, 0.5, "cuda:0", 10
N = 2 * B + 7
x, y = (torch.from_numpy(a) for a in make_cifar_like(4 * B, seed=5))
xe, ye = (torch.from_numpy(a) for a in make_cifar_like(N, seed=6))


def trainer(seed=2, **kw):
    tr = FusedResNetTrainer(batch=B, device=DEV, seed=seed, **kw)
    tr.load_shard(x, y)
    return tr


def state(tr) -> dict:
    d = {"params": tr.params, "shadow": tr.shadow, "mom": tr.mom, "ema": tr.ema, "ema_step": tr.ema_step,
         "ema_ticket": tr.ema_ticket, "cursor": tr.cursor, "fc_wt": tr.fc_wt, "grad": tr.grad}
    d.update({f"wt/{name}": c.wt for name, c in tr.conv.items()})
    for name, (rm, rv) in tr.running_stats().items():
        d[f"bn/{name}/mean"], d[f"bn/{name}/var"] = rm, rv
    return {k: v for k, v in d.items() if v is not None}


def same(a: dict, b: dict) -> list:
    return sorted(k for k in a if not torch.equal(a[k], b[k]))


def raises(fn) -> bool:
    try:
        fn()
    except ValueError:
        return True
    return False


out = {"deterministic_build": K.deterministic()}
tr, twin = trainer(ema_decay=D), trainer(ema_decay=D)
for t in (tr, twin):
    t.capture(warmup=2)  # two eager steps, then the capture
    t.step()
    t.step()
torch.cuda.synchronize()
out["captured"] = tr.graph is not None and twin.graph is not None

before = {k: v.clone() for k, v in state(tr).items()}
ptrs = {k: v.data_ptr() for k, v in state(tr).items()}
keep_xyc = (tr.x.data_ptr(), tr.y.data_ptr(), tr.cursor.data_ptr())
rep = tr.evaluate_full(xe, ye, topk=5)
cache = tr._eval_cache[2].data_ptr()
rep2 = tr.evaluate_full(xe, ye, topk=5)
rep1 = tr.evaluate_full(xe, ye, topk=1)
rep_ema = tr.evaluate_full(xe, ye, ema=True, topk=5)
torch.cuda.synchronize()
after = state(tr)
out["state"] = {"changed": same(before, after), "tensors": len(before),
                "no_tensor_moved": all(after[k].data_ptr() == p for k, p in ptrs.items()),
                "shard_and_cursor_restored": (tr.x.data_ptr(), tr.y.data_ptr(), tr.cursor.data_ptr()) == keep_xyc,
                "graph_kept": tr.graph is not None}

# the graph captured before the evaluations replays after them: the twin never evaluated
for t in (tr, twin):
    for _ in range(3):
        t.step()
torch.cuda.synchronize()
out["graph"] = {"changed_vs_twin": same(state(tr), state(twin)), "cursor": int(tr.cursor.item())}

# the engine's own logits and loss rows for the padded set, batch by batch
rows = (N + B - 1) // B * B
xp = torch.zeros(rows, 32, 32, 3, dtype=torch.uint8, device=DEV)
yp = torch.zeros(rows, dtype=torch.uint8, device=DEV)
xp[:N].copy_(xe.reshape(N, 32, 32, 3))
yp[:N].copy_(ye)
saved = (tr.x, tr.y, tr.cursor)
tr.x, tr.y, tr.cursor = xp, yp, torch.zeros(1, dtype=torch.int32, device=DEV)
logits, loss = [], []
for _ in range(rows // B):
    tr.forward_eval()
    logits.append(tr.logits.clone())
    loss.append(tr.loss.clone())
    K.cursor_bump(tr.cursor)
tr.x, tr.y, tr.cursor = saved
logits, loss = torch.cat(logits).cpu(), torch.cat(loss).cpu()
# (three replays later: the reports are compared with the weights as they are now)
now = tr.evaluate_full(xe, ye, topk=5)
want = eval_reference(logits[:N], ye, loss[:N], NCLS, 5)
want1 = eval_reference(logits[:N], ye, loss[:N], NCLS, 1)
out["report"] = {"n": rep.n, "N": N, "equals_reference": now == want, "topk1_equals_reference":
                 tr.evaluate_full(xe, ye, topk=1) == want1, "second_call_identical": rep == rep2,
                 "topk1_is_top1": rep1.topk == rep1.top1 == rep.top1, "cache_reused": tr._eval_cache[2].data_ptr() == cache,
                 "confusion_sum": int(now.confusion.sum()), "good": now.n - now.bad,
                 "padding_rows_nonzero_logits": bool((logits[N:] != 0).any()),
                 "now": {k: v for k, v in now.as_dict().items() if k != "confusion"}}

# ema=True against a second engine holding the average, with the same running statistics
second = trainer(seed=9)
second.set_flat(tr.ema_flat())
for name, (rm, rv) in tr.running_stats().items():
    second.running_stats()[name][0].copy_(rm)
    second.running_stats()[name][1].copy_(rv)
avg = tr.evaluate_full(xe, ye, ema=True, topk=5)
out["ema"] = {"equals_second_engine": avg == second.evaluate_full(xe, ye, topk=5), "n": avg.n,
              "differs_from_live": avg != now, "first_differs_from_live": rep_ema != rep}
empty = (xe[:0], ye[:0])
out["refusals"] = {"topk0": raises(lambda: tr.evaluate_full(xe, ye, topk=0)),
                   "topk11": raises(lambda: tr.evaluate_full(xe, ye, topk=NCLS + 1)),
                   "empty": raises(lambda: tr.evaluate_full(*empty)),
                   "ema_without_ema": raises(lambda: second.evaluate_full(xe, ye, ema=True))}
print(json.dumps(out))
