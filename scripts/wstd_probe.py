"""Step time of the ResNet engine with weight_std on against off on one GPU: the two trainers'
captured steps timed in alternating windows (device events around each window), so clock drift
hits both alike; then the two grouped launches alone, back to back over ResNet-18's plan, with the
bytes the plan says they move.  Prints one JSON line.

    python scripts/wstd_probe.py [--batch 1024] [--norm batch] [--steps 20] [--rounds 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/wstd_probe.py --kernels-only
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def plan_bytes(plan) -> dict:
    """Bytes each launch reads and writes, from the plan: the forward reads w (4 B) and writes bf16
    (2 B) per element, the backward reads w and G and writes G."""
    n = int((plan.tensors_h[:, 1].astype("int64") * plan.tensors_h[:, 2]).sum())
    return {"elements": n, "rows": plan.rows, "workgroups": plan.n_work, "fwd": {"read": 4 * n, "write": 2 * n},
            "bwd": {"read": 8 * n, "write": 4 * n}}


def time_kernels(iters: int) -> dict:
    from serverless_learn_amd.models.resnet import WS_EPS, init_params, resnet18_spec
    from serverless_learn_amd.ops import cnn as K

    spec = resnet18_spec()
    plan = K.wstd_plan(spec.convs(), "cuda:0")
    w = init_params(spec, 0).to("cuda:0")
    sh, g = torch.zeros_like(w, dtype=torch.bfloat16), torch.randn_like(w)
    out = plan_bytes(plan)
    for name, fn in (("fwd", lambda: K.wstd_fwd(w, sh, plan, eps=WS_EPS)), ("bwd", lambda: K.wstd_bwd(w, g, plan, eps=WS_EPS))):
        for _ in range(5):
            fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        us = 1e3 * t0.elapsed_time(t1) / iters
        out[name].update(us_back_to_back=us, gb_per_s=(out[name]["read"] + out[name]["write"]) / us / 1e3)
    return out


def main() -> int:
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--norm", default="batch")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    res = {"kernels": time_kernels(a.kernel_iters)}
    if a.kernels_only:
        print(json.dumps(res))
        return 0
    x, y = (torch.from_numpy(t) for t in make_cifar_like(2 * a.batch, seed=1))
    trs = {k: FusedResNetTrainer(batch=a.batch, device="cuda:0", norm=a.norm, weight_std=k == "on") for k in ("off", "on")}
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
    res.update(batch=a.batch, norm=a.norm, steps_per_window=a.steps, step_ms=ms, median_ms=med,
               on_minus_off_ms=med["on"] - med["off"], loss={k: tr.stats().loss for k, tr in trs.items()})
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
