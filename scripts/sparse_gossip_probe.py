"""Numbers for the top-k sparse gossip exchange (profiles/r10_sparse/README.md).

  speed     on the GPU: wall time of GossipState.make_sparse_delta (select -> host arrays in hand)
            against the dense make_delta() + encode_update, interleaved, at the MLP's and
            ResNet-18's parameter counts; wire bytes per message; device time of the select alone.
  accuracy  two MLP trainers on different shards that exchange every --every steps, dense and at
            each --topk: the loss of both after --steps steps, on their last batch and on a held-out
            shard (same seeds; CPU trainers by default).

usage: python scripts/sparse_gossip_probe.py speed|accuracy [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from serverless_learn_amd.models.mlp import N_PARAMS  # noqa: E402
from serverless_learn_amd.parallel.gossip import GossipState  # noqa: E402
from serverless_learn_amd.wire import codec  # noqa: E402


def _spread(xs):
    return {"median_ms": round(statistics.median(xs) * 1e3, 3), "min_ms": round(min(xs) * 1e3, 3),
            "max_ms": round(max(xs) * 1e3, 3), "reps": len(xs)}


def speed(args) -> dict:
    if not torch.cuda.is_available():
        raise SystemExit("speed needs the GPU: a CPU timing says nothing about it")
    from serverless_learn_amd.models.resnet import resnet18_spec

    dev = torch.device("cuda", 0)
    sizes = {"mlp": N_PARAMS, "resnet18": int(resnet18_spec().n_flat)}
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": []}
    for name, n in sizes.items():
        gen = torch.Generator(device="cpu").manual_seed(1)
        m = torch.randn(n, generator=gen).to(dev)
        step = (torch.randn(n, generator=gen) * 0.01).to(dev)  # the progress since the last exchange
        g = GossipState(m, 0.5)

        def dense():
            g.model.add_(step)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            msg = codec.encode_update(g.make_delta())
            dt = time.perf_counter() - t0
            g.old.copy_(g.model)
            return dt, len(msg)

        def sparse(k):
            g.old.copy_(g.model)
            g.model.add_(step)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            index, value = g.make_sparse_delta(k)
            t1 = time.perf_counter()
            msg = codec.encode_sparse_update(index, value, n)
            t2 = time.perf_counter()
            return t1 - t0, t2 - t0, len(msg), int(index.size)

        def select_device_ms(k):
            from serverless_learn_amd.ops import _native as N

            g.old.copy_(g.model)
            g.model.add_(step)
            o = g._topk_out
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            N.call("sl_gossip_topk", N.ptr(g.model), N.ptr(g.old), n, k, N.ptr(o[4:4 + k]), N.ptr(o[4 + k:4 + 2 * k]),
                   N.ptr(o), N.ptr(g._topk_ws), N.stream_ptr())
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        ks = {x: max(1, math.ceil(x * n)) for x in args.topk}
        for _ in range(2):  # warm every shape
            dense()
            for k in ks.values():
                sparse(k)
                select_device_ms(k)
        td, ts, tse, tk = [], {x: [] for x in ks}, {x: [] for x in ks}, {x: [] for x in ks}
        nbytes = {}
        for _ in range(args.reps):  # interleaved: dense, then each k
            dt, nbytes["dense"] = dense()
            td.append(dt)
            for x, k in ks.items():
                a, b, nbytes[x], count = sparse(k)
                assert count == k, (count, k)
                ts[x].append(a)
                tse[x].append(b)
            for x, k in ks.items():
                tk[x].append(select_device_ms(k))
        case = {"model": name, "n": n, "dense_make_delta_plus_encode": _spread(td), "dense_wire_bytes": nbytes["dense"],
                "sparse": {}}
        for x, k in ks.items():
            case["sparse"][str(x)] = {"k": k, "make_sparse_delta": _spread(ts[x]),
                                      "make_sparse_delta_plus_encode": _spread(tse[x]),
                                      "select_kernels_device": _spread(tk[x]), "wire_bytes": nbytes[x],
                                      # algorithm bytes of the select: m, o (8) + the delta written once (4)
                                      # and read by four passes (16)
                                      "select_bytes_per_element_by_design": 28}
        out["cases"].append(case)
    return out


def accuracy(args) -> dict:
    from serverless_learn_amd.data.synthetic import make_mnist_like
    from serverless_learn_amd.models import make_trainer

    from serverless_learn_amd.models.mlp import reference_grads

    dev = torch.device(args.device)
    shards = [make_mnist_like(args.records, seed=s) for s in (0, 1)]
    held = make_mnist_like(args.records, seed=2)  # seen by neither worker
    hx, hy = torch.from_numpy(held[0]), torch.from_numpy(held[1])
    out = {"device": str(dev), "steps": args.steps, "every": args.every, "batch": args.batch, "runs": []}
    for x in [0.0] + list(args.topk):
        trs, gs = [], []
        for w in range(2):
            tr = make_trainer("mlp", dev, batch=args.batch, lr=0.05, momentum=0.9, weight_decay=0.0, seed=0,
                              world_size=1)
            tr.load_shard(torch.from_numpy(shards[w][0]).to(dev), torch.from_numpy(shards[w][1]).to(dev))
            trs.append(tr)
            gs.append(GossipState(tr.params[:tr.n_params], 0.5))
        k = max(1, math.ceil(x * N_PARAMS)) if x > 0 else 0
        wire = 0
        for s in range(1, args.steps + 1):
            for tr in trs:
                tr.step()
            if s % args.every == 0:
                a, b = (gs[0], gs[1]) if (s // args.every) % 2 else (gs[1], gs[0])  # take turns to initiate
                if k:
                    i, v = a.make_sparse_delta(k)
                    ri, rv = b.serve_sparse(i, v, k, sparse_len=N_PARAMS)
                    a.absorb_sparse(ri, rv)
                    wire += len(codec.encode_sparse_update(i, v, N_PARAMS)) + len(
                        codec.encode_sparse_update(ri, rv, N_PARAMS))
                else:
                    d = a.make_delta()
                    r = b.serve(d)
                    a.absorb(r, d)
                    wire += 8 * (d.size + r.size)
                for tr in trs:
                    tr.refresh_shadows()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        st = [tr.stats() for tr in trs]
        ev = [reference_grads(tr.params[:tr.n_params].detach().cpu(), hx, hy) for tr in trs]
        resid = [float((g.model.double() - g.old.double()).abs().sum() / g.model.double().abs().sum()) for g in gs]
        out["runs"].append({"gossip_topk": x, "k": k, "loss": [round(s.loss, 5) for s in st],
                            "accuracy": [round(s.accuracy, 4) for s in st],
                            "heldout_loss": [round(float(e[0]) / hy.numel(), 5) for e in ev],
                            "heldout_accuracy": [round(float(e[1]) / hy.numel(), 4) for e in ev],
                            "wire_bytes_total": wire,
                            "unsent_residual_l1_over_model_l1": [round(r, 5) for r in resid]})
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["speed", "accuracy"])
    ap.add_argument("--topk", type=float, nargs="+", default=[0.01, 0.1])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--records", type=int, default=8192)
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    res = speed(args) if args.what == "speed" else accuracy(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
