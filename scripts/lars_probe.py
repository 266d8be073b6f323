"""What optimizer="lars" costs on one GPU.  Prints one JSON line.

* ``launch_us``: LARS's three launches over a ResNet-18 trainer's own vectors (11.2 M parameters), each timed
  back to back between device events, beside ``sl_clip_grad_norm`` at ``max_norm = inf`` (its sum-of-squares
  launch, which reads half the bytes of the norms launch, plus a scale launch that exits after the fold) and the
  ungrouped ``sl_sgd_flat_lr`` update.
* ``step_ms``: the captured step under ``lars`` against ``sgd`` with the same schedule, in alternating windows,
  so clock drift hits both alike.

    python scripts/lars_probe.py [--batch 1024] [--steps 20] [--rounds 5] [--reps 200]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps: int) -> float:
    """Microseconds per call of ``fn`` over ``reps`` back-to-back calls (after 10 warm-up calls)."""
    for _ in range(10):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return 1e3 * t0.elapsed_time(t1) / reps


def main() -> int:
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer
    from serverless_learn_amd.ops import optim as O

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    sched = dict(weight_decay=5e-4, lr_schedule="cosine", lr_warmup_steps=5, lr_decay_steps=100_000)
    x, y = (torch.from_numpy(t) for t in make_cifar_like(2 * a.batch, seed=1))
    trs = {k: FusedResNetTrainer(batch=a.batch, device="cuda:0", optimizer=k, **sched) for k in ("sgd", "lars")}
    for tr in trs.values():
        tr.load_shard(x, y)
        tr.step()
    torch.cuda.synchronize()
    # the launches alone, on the LARS trainer's vectors (lr 0 from here on: the weights stay where they are)
    tr, s = trs["lars"], trs["lars"].opt
    b, zero, mom = tr.lars_buf, torch.zeros(1, device="cuda:0"), tr.mom.clone()  # (a scratch momentum)
    partials, norm = O.clip_buffers(tr.n_params, tr.device)
    n_bytes = 4 * int(sum(t[1] for t in b.plan.tensors.tolist()))
    launch_us = {
        "sl_lars_norms": _timed(lambda: O.lars_norms(tr.params, tr.grad, b), a.reps),
        "sl_lars_trust": _timed(lambda: O.lars_trust(b, s.lars_eta, s.lars_eps, s.weight_decay), a.reps),
        "sl_sgd_flat_lars": _timed(lambda: O.sgd_flat_lars(tr.params, tr.grad, mom, tr.opt_step, zero, b, s.decays(),
                                                           momentum=0.9, shadow=tr.shadow), a.reps),
        "sl_clip_grad_norm(inf)": _timed(lambda: O.clip_grad_norm_flat(tr.grad, float("inf"), partials, norm), a.reps),
        "sl_sgd_flat_lr": _timed(lambda: O.sgd_flat_lr(tr.params, tr.grad, mom, tr.opt_step, zero, 0.9,
                                                       s.weight_decay, shadow=tr.shadow), a.reps),
    }
    for t in trs.values():
        t.capture(warmup=3)
        for _ in range(a.steps):
            t.step()
    torch.cuda.synchronize()
    ms = {k: [] for k in trs}
    for _ in range(a.rounds):
        for k, t in trs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                t.step()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1) / a.steps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"batch": a.batch, "n_params": tr.n_params, "chunks": len(b.plan.chunks),
                      "tensors": len(b.plan.names), "reps": a.reps, "launch_us": launch_us,
                      "norms_gb_s": 2 * n_bytes / launch_us["sl_lars_norms"] / 1e3,
                      "clip_gb_s": 4 * tr.n_params / launch_us["sl_clip_grad_norm(inf)"] / 1e3,
                      "steps_per_window": a.steps, "step_ms": ms, "median_ms": med,
                      "lars_over_sgd": med["lars"] / med["sgd"], "loss": {k: t.stats().loss for k, t in trs.items()}}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
