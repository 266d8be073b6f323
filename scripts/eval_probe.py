#!/usr/bin/env python
"""What held-out evaluation costs (profiles/r17_eval).

Four measurements, each a process of its own so that each runs under its own time limit:

    timeout -k 10 200 python scripts/eval_probe.py kernel --out profiles/r17_eval && \\
    timeout -k 10 200 python scripts/eval_probe.py mlp --out profiles/r17_eval && \\
    timeout -k 10 400 python scripts/eval_probe.py resnet --out profiles/r17_eval && \\
    timeout -k 10 300 python scripts/eval_probe.py worker --out profiles/r17_eval

kernel  sl_eval_accum alone at 1024 and 65,536 rows of ten classes: device events around 200 launches,
        several rounds.  Microseconds per launch.
mlp     evaluate_full against evaluate() on the same 10,000 records (evaluate() covers the 9,984 in whole
        64-row blocks): wall clock from a drained device to the returned result, alternating, the
        median of several runs after a warm-up.
resnet  the same for ResNet-18 at B = 1024 on 10,000 records (evaluate() covers 9 whole batches, 9,216
        records; evaluate_full 10 batches, the last with 784 valid rows), the live weights and ema=True.
worker  a training worker at the default settings (the MLP, batch 1024, 10,000 held-out records, top-5)
        with eval_every on: the `secs` of its `eval` events, which is how long the training loop stood
        still for each evaluation (the chunks queued before it drain inside that time).

Each prints one JSON line and writes it to <out>/eval_probe_<what>.json.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RECORDS = 10_000


def _summary(v, unit="ms", digits=4):
    return {f"{unit}_runs": [round(t, digits) for t in v], f"{unit}_min": round(min(v), digits),
            f"{unit}_max": round(max(v), digits), f"{unit}_median": round(statistics.median(v), digits)}


def _wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _alternate(fns: dict, runs: int) -> dict:
    for fn in fns.values():  # warm-up: workspaces, the padded copy, the EMA's shadows
        fn()
        fn()
    ms = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            ms[name].append(_wall(fn))
    return {name: _summary(v) for name, v in ms.items()}


def kernel(args) -> dict:
    from serverless_learn_amd.ops import evalmetrics as E

    dev = torch.device("cuda:0")
    res = {"what": "kernel", "launches": args.launches, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    for rows in (1024, 65536):
        g = torch.Generator().manual_seed(rows)
        z = torch.randn(rows, 10, generator=g).to(dev)
        lab = torch.randint(0, 10, (rows,), generator=g).to(torch.uint8).to(dev)
        loss = torch.rand(rows, generator=g).to(dev)
        acc = E.new_acc(dev)
        fn = lambda: E.eval_accum(z, lab, loss, rows, 10, 5, acc)  # noqa: E731
        for _ in range(20):
            fn()
        us = []
        for _ in range(args.rounds):
            acc.zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                fn()
            b.record()
            b.synchronize()
            us.append(1e3 * a.elapsed_time(b) / args.launches)
        res[str(rows)] = dict(_summary(us, "us", 3), n=int(acc[0].item()), workgroups=(rows + 15) // 16)
    return res


def mlp(args) -> dict:
    from serverless_learn_amd.data.device_synth import synth_on_device
    from serverless_learn_amd.models.mlp import FusedMLPTrainer

    dev = torch.device("cuda:0")
    x, y = synth_on_device("mnist", RECORDS, seed=1, device=dev)
    tr = FusedMLPTrainer(batch=1024, device=dev, seed=0, ema_decay=0.999)
    res = {"what": "mlp", "records": RECORDS, "runs": args.runs, "device": torch.cuda.get_device_name(0)}
    res.update(_alternate({"evaluate": lambda: tr.evaluate(x, y), "evaluate_full": lambda: tr.evaluate_full(x, y),
                           "evaluate_full_ema": lambda: tr.evaluate_full(x, y, ema=True)}, args.runs))
    rep, old = tr.evaluate_full(x, y), tr.evaluate(x, y)
    res["covered"] = {"evaluate": old.n, "evaluate_full": rep.n}
    res["loss"] = {"evaluate": old.loss, "evaluate_full": rep.loss}
    return res


def resnet(args) -> dict:
    from serverless_learn_amd.data.device_synth import synth_on_device
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    dev = torch.device("cuda:0")
    B = 1024
    x, y = synth_on_device("cifar", RECORDS, seed=1, device=dev)
    tr = FusedResNetTrainer(batch=B, device=dev, seed=0, ema_decay=0.999)
    res = {"what": "resnet", "batch": B, "records": RECORDS, "runs": args.runs, "device": torch.cuda.get_device_name(0)}
    res.update(_alternate({"evaluate": lambda: tr.evaluate(x, y), "evaluate_full": lambda: tr.evaluate_full(x, y),
                           "evaluate_full_ema": lambda: tr.evaluate_full(x, y, ema=True)}, args.runs))
    rep, old = tr.evaluate_full(x, y), tr.evaluate(x, y)
    res["covered"] = {"evaluate": old.n, "evaluate_full": rep.n}
    res["ms_per_batch"] = {"evaluate": round(res["evaluate"]["ms_median"] / (old.n // B), 4),
                           "evaluate_full": round(res["evaluate_full"]["ms_median"] / ((rep.n + B - 1) // B), 4)}
    return res


def worker(args) -> dict:
    from serverless_learn_amd.runtime.local_cluster import LocalCluster, fast_config
    from serverless_learn_amd.utils.log import Logger

    events, emit = [], Logger._emit

    def tap(self, level, event, **f):
        if event in ("eval", "eval_skipped", "eval_failed", "train"):
            events.append((event, f))
        emit(self, level, event, **f)

    Logger._emit = tap
    every, steps = 400, 2400
    # the defaults of Config for everything evaluation reads: model, batch, eval_records, eval_topk
    c = LocalCluster(fast_config(device="cuda:0", batch=1024, shard_records=65536, log_every=200, eval_every=every,
                                 ema_decay=args.ema_decay, max_steps=steps))
    try:
        w = c.add_worker()
        w.hold_at = 0
        ok = c.wait_for(lambda: w.held_step == 0 and w._eval_shard is not None, timeout=120)
        w.hold_at = None
        ok = ok and c.wait_for(lambda: w.state == "done", timeout=200)
    finally:
        c.stop()
    evals = [f for e, f in events if e == "eval"]
    secs = [f["secs"] for f in evals]
    trains = [f for e, f in events if e == "train"]
    return {"what": "worker", "ok": bool(ok), "model": c.cfg.model, "batch": c.cfg.batch,
            "eval_records": c.cfg.eval_records, "eval_topk": c.cfg.eval_topk, "eval_every": every, "steps": steps,
            "ema_decay": args.ema_decay, "evaluations": len(evals),
            "skipped_or_failed": len([e for e, f in events if e in ("eval_skipped", "eval_failed")]),
            "pause": _summary([1e3 * s for s in secs[1:]] or [0.0]), "first_pause_ms": round(1e3 * secs[0], 3) if secs else None,
            "step_ms": [f.get("step_ms") for f in trains][-3:], "last": evals[-1] if evals else None,
            "device": torch.cuda.get_device_name(0)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "mlp", "resnet", "worker"])
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--ema-decay", type=float, default=0.0)
    args = ap.parse_args(argv)
    res = {"kernel": kernel, "mlp": mlp, "resnet": resnet, "worker": worker}[args.what](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        name = f"eval_probe_{args.what}" + ("_ema" if args.what == "worker" and args.ema_decay else "")
        with open(os.path.join(args.out, name + ".json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
