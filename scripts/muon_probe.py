"""What optimizer="muon" costs on one GPU.  Prints one JSON line.

* ``launch_us``: the Muon update's launches at ResNet-18's real plan (19 tensors, 11.2 M elements), each timed back
  to back between device events, with the achieved TFLOP/s of the Gram and apply launches (nominal ``2 m^2 n``
  operations per tensor; the Gram launch computes only the tiles on or below the diagonal).
* ``ns_us``: one whole orthogonalisation (prep + 5 x (gram, poly, apply)) through the grouped launches against the
  same iteration written with ``torch.matmul`` in bf16, one tensor at a time, in alternating rounds in this process.
* ``step_ms``: the captured step under ``muon`` against ``sgd`` with the same schedule, in alternating windows.

    python scripts/muon_probe.py [--batch 1024] [--steps 20] [--rounds 5] [--reps 50]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps: int) -> float:
    """Microseconds per call of ``fn`` over ``reps`` back-to-back calls (after 5 warm-up calls)."""
    for _ in range(5):
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
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    sched = dict(weight_decay=5e-4, lr_schedule="cosine", lr_warmup_steps=5, lr_decay_steps=100_000)
    x, y = (torch.from_numpy(t) for t in make_cifar_like(2 * a.batch, seed=1))
    trs = {k: FusedResNetTrainer(batch=a.batch, device="cuda:0", optimizer=k, **sched) for k in ("sgd", "muon")}
    for tr in trs.values():
        tr.load_shard(x, y)
        tr.step()
    torch.cuda.synchronize()
    # the launches alone, on the Muon trainer's gradient and a scratch momentum (lr 0: the weights stay)
    tr, s = trs["muon"], trs["muon"].opt
    b, zero, mom = tr.muon_buf, torch.zeros(1, device="cuda:0"), tr.mom.clone()
    O.muon_prep(tr.grad, mom, b, 0.9)
    launch_us = {
        "sl_muon_prep": _timed(lambda: O.muon_prep(tr.grad, mom, b, 0.0), a.reps),  # (mu 0: mom stays g)
        "sl_muon_gram": _timed(lambda: O.muon_gram(b, 0), a.reps),
        "sl_muon_poly": _timed(lambda: O.muon_poly(b), a.reps),
        "sl_muon_apply": _timed(lambda: O.muon_apply(b, 0), a.reps),
        "sl_sgd_flat_muon": _timed(lambda: O.sgd_flat_muon(tr.params, tr.grad, mom, tr.opt_step, zero, b, s.decays(),
                                                           momentum=0.0, shadow=tr.shadow), a.reps),
        "sl_sgd_flat_lr": _timed(lambda: O.sgd_flat_lr(tr.params, tr.grad, mom, tr.opt_step, zero, 0.0,
                                                       s.weight_decay, shadow=tr.shadow), a.reps),
    }
    shapes = [(min(m, n), max(m, n)) for _, m, n, *_ in b.plan.tensors.tolist()]
    gemm_flop = sum(2.0 * m * m * n for m, n in shapes)
    # the same iteration through torch.matmul, one tensor at a time, on the same X0
    O.muon_prep(tr.grad, mom, b, 0.0)
    x0 = [b.x[0][r[4]:r[4] + r[1] * r[2]].view(m, n).clone() for r, (m, n) in zip(b.plan.tensors.tolist(), shapes)]
    ca, cb, cc = O.NS_COEFFS

    def matmul_loop():
        for X in x0:
            for _ in range(5):
                A = X @ X.T
                X = ca * X + (cb * A + cc * (A @ A)) @ X

    def grouped():
        O.muon_orthogonalize(tr.grad, mom, b, 0.0, True, 5)

    ns = {"grouped": [], "torch_matmul": []}
    for _ in range(a.rounds):
        ns["grouped"].append(_timed(grouped, a.reps))
        ns["torch_matmul"].append(_timed(matmul_loop, a.reps))
    ns_med = {k: statistics.median(v) for k, v in ns.items()}
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
    print(json.dumps({"batch": a.batch, "n_params": tr.n_params, "tensors": len(b.plan.names), "reps": a.reps,
                      "workgroups": {"prep": [len(b.plan.chunks), len(b.plan.tiles)],
                                     "gram": [len(b.plan.gram_tiles), len(b.plan.tri_tiles)],
                                     "poly": len(b.plan.poly_tiles), "apply": len(b.plan.tiles)},
                      "launch_us": launch_us, "gemm_gflop": gemm_flop / 1e9,
                      "gram_tflops": gemm_flop / launch_us["sl_muon_gram"] / 1e6,
                      "apply_tflops": gemm_flop / launch_us["sl_muon_apply"] / 1e6,
                      "ns_us": ns, "ns_median_us": ns_med, "grouped_over_matmul": ns_med["grouped"] / ns_med["torch_matmul"],
                      "steps_per_window": a.steps, "step_ms": ms, "median_ms": med,
                      "muon_over_sgd": med["muon"] / med["sgd"], "loss": {k: t.stats().loss for k, t in trs.items()}}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
