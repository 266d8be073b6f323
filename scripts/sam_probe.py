"""What sam_rho costs on one GPU.  Prints one JSON line.

* ``launch_us``: ``sl_sam_norms``, ``sl_sam_scale``, ``sl_sam_perturb`` and the restoring ``sl_accum_flat`` over a
  ResNet-18 trainer's own vectors (11.2 M parameters, 2,729 chunks), plain and adaptive, back to back between device
  events, beside one momentum-SGD update launch (``sl_sgd_flat``) on the same vectors.  A perturbed vector is not
  perturbed twice: the perturb arm is timed as perturb + restore with the restore's own time subtracted.
* ``step_ms``: the captured step with ``sam_rho`` on against the same step with it off (what a trainer launched
  before the option existed), in alternating windows, so clock drift hits both alike.

    python scripts/sam_probe.py [--batch 1024] [--steps 20] [--rounds 5] [--reps 200]
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
    ap.add_argument("--rho", type=float, default=0.05)
    a = ap.parse_args()
    x, y = (torch.from_numpy(t) for t in make_cifar_like(2 * a.batch, seed=1))
    trs = {k: FusedResNetTrainer(batch=a.batch, device="cuda:0", weight_decay=5e-4, **kw)
           for k, kw in (("off", {}), ("sam", dict(sam_rho=a.rho)), ("asam", dict(sam_rho=a.rho, sam_adaptive=True)))}
    for tr in trs.values():
        tr.load_shard(x, y)
        tr.step()
    torch.cuda.synchronize()
    tr = trs["sam"]
    b, eta = tr.sam_buf, tr.opt.sam_eta
    w, g, sh, mom = tr.params.clone(), tr.grad.clone(), tr.shadow.clone(), tr.mom.clone()
    restore_us = _timed(lambda: O.sam_restore(w, b), a.reps)
    launch_us = {"sl_accum_flat(restore)": restore_us, "sl_sam_scale": _timed(lambda: O.sam_scale(b, a.rho), a.reps),
                 "sl_sgd_flat": _timed(lambda: O.sgd_flat(w, g, mom, 0.0, 0.9, 5e-4, shadow=sh), a.reps)}
    for name, ad in (("plain", False), ("adaptive", True)):
        launch_us[f"sl_sam_norms({name})"] = _timed(lambda: O.sam_norms(w, g, b, ad, eta), a.reps)
        launch_us[f"sl_sam_perturb({name})"] = _timed(
            lambda: (O.sam_perturb(w, g, sh, b, ad, eta), O.sam_restore(w, b)), a.reps) - restore_us
    n = tr.n_params
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
    print(json.dumps({"batch": a.batch, "n_params": n, "chunks": int(b.partials.numel()), "reps": a.reps,
                      "launch_us": launch_us,
                      "norms_plain_gb_s": 4 * n / launch_us["sl_sam_norms(plain)"] / 1e3,
                      "norms_adaptive_gb_s": 8 * n / launch_us["sl_sam_norms(adaptive)"] / 1e3,
                      "perturb_plain_gb_s": 18 * n / launch_us["sl_sam_perturb(plain)"] / 1e3,
                      "steps_per_window": a.steps, "step_ms": ms, "median_ms": med,
                      "sam_over_off": med["sam"] / med["off"], "asam_over_off": med["asam"] / med["off"],
                      "rho": a.rho, "sam_stats": {k: t.sam_stats() for k, t in trs.items() if k != "off"},
                      "loss": {k: t.stats().loss for k, t in trs.items()}}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
