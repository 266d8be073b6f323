"""What agc_clip costs on one GPU.  Prints one JSON line.

* ``launch_us``: ``sl_agc_clip`` over a ResNet-18 trainer's own vectors (11.2 M parameters, 4,840 units) at a clip
  where no unit is clipped (the launch only reads) and at one where every unit is (it also writes the gradient back),
  back to back between device events, beside ``sl_wstd_bwd`` and ``sl_clip_grad_norm`` at ``max_norm = inf`` on the
  same vectors.  A clipped gradient is not clipped twice, so the all-clip arm restores the gradient with a device copy
  before every call; ``copy`` is that copy alone, already subtracted from ``all_clip``.
* ``step_ms``: the captured step with ``agc_clip`` on against the same step with it off (what a trainer launched
  before the option existed), in alternating windows, so clock drift hits both alike.

    python scripts/agc_probe.py [--batch 1024] [--steps 20] [--rounds 5] [--reps 200]
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
    from serverless_learn_amd.models.resnet import WS_EPS
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer
    from serverless_learn_amd.ops import cnn as K
    from serverless_learn_amd.ops import optim as O

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--clip", type=float, default=0.02)
    a = ap.parse_args()
    x, y = (torch.from_numpy(t) for t in make_cifar_like(2 * a.batch, seed=1))
    trs = {k: FusedResNetTrainer(batch=a.batch, device="cuda:0", weight_decay=5e-4, agc_clip=c)
           for k, c in (("off", 0.0), ("agc", a.clip))}
    for tr in trs.values():
        tr.load_shard(x, y)
        tr.step()
    torch.cuda.synchronize()
    tr = trs["agc"]
    b, g0, g = tr.agc_buf, tr.grad.clone(), tr.grad.clone()
    wstd = K.wstd_plan(tr.spec.convs(), tr.device)
    partials, norm = O.clip_buffers(tr.n_params, tr.device)
    copy_us = _timed(lambda: g.copy_(g0), a.reps)
    launch_us = {
        "none_clip": _timed(lambda: O.agc_clip_flat(tr.params, g, b, 1e30), a.reps),
        "all_clip": _timed(lambda: (g.copy_(g0), O.agc_clip_flat(tr.params, g, b, 1e-30)), a.reps) - copy_us,
        "copy": copy_us,
        "sl_wstd_bwd": _timed(lambda: K.wstd_bwd(tr.params, g, wstd, eps=WS_EPS), a.reps),
        "sl_clip_grad_norm(inf)": _timed(lambda: O.clip_grad_norm_flat(g, float("inf"), partials, norm), a.reps),
    }
    O.agc_clip_flat(tr.params, g.copy_(g0), b, 1e-30)
    torch.cuda.synchronize()
    all_clipped = int((b.stats[:, 2] < 1).sum())
    unit_bytes = 4 * int(b.plan.units[:, 1].sum())
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
    stats = tr.agc_stats()
    print(json.dumps({"batch": a.batch, "n_params": tr.n_params, "units": len(b.plan.units), "unit_bytes": unit_bytes,
                      "reps": a.reps, "launch_us": launch_us, "all_clip_units": all_clipped,
                      "none_clip_gb_s": 2 * unit_bytes / launch_us["none_clip"] / 1e3,
                      "all_clip_gb_s": 3 * unit_bytes / launch_us["all_clip"] / 1e3,
                      "steps_per_window": a.steps, "step_ms": ms, "median_ms": med,
                      "agc_over_off": med["agc"] / med["off"], "clip": a.clip,
                      "clipped_units_last_step": sum(c for _, c, _ in stats.values()),
                      "loss": {k: t.stats().loss for k, t in trs.items()}}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
