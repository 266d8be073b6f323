"""Step time of the ResNet engine under norm="group" against norm="batch" on one GPU: the two
trainers' captured steps timed in alternating windows (device events around each window), so
clock drift hits both alike.  Prints one JSON line.

    python scripts/groupnorm_probe.py [--batch 1024] [--groups 32] [--steps 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    x, y = (torch.from_numpy(t) for t in make_cifar_like(2 * a.batch, seed=1))
    trs = {"batch": FusedResNetTrainer(batch=a.batch, device="cuda:0"),
           "group": FusedResNetTrainer(batch=a.batch, device="cuda:0", norm="group", norm_groups=a.groups)}
    for tr in trs.values():
        tr.load_shard(x, y)
        tr.capture(warmup=3)
        for _ in range(a.steps):
            tr.step()
    torch.cuda.synchronize()
    ms = {k: [] for k in trs}
    for _ in range(a.rounds):
        for k, tr in trs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                tr.step()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1) / a.steps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"batch": a.batch, "groups": a.groups, "steps_per_window": a.steps, "step_ms": ms,
                      "median_ms": med, "group_over_batch": med["group"] / med["batch"],
                      "loss": {k: tr.stats().loss for k, tr in trs.items()}}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
