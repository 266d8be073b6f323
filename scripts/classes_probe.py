#!/usr/bin/env python
"""What a classifier head of more than 16 classes costs (profiles/r18_classes).

Each measurement is a process of its own, so that each runs under its own time limit:

    for r in 4 8 16 32; do SL_CE_WIDE_ROWS=$r timeout -k 10 120 python scripts/classes_probe.py loss \\
        --out profiles/r18_classes --tag rows$r || break; done
    timeout -k 10 120 python scripts/classes_probe.py eval --out profiles/r18_classes && \\
    timeout -k 10 120 python scripts/classes_probe.py fc --out profiles/r18_classes && \\
    timeout -k 10 400 python scripts/classes_probe.py step --out profiles/r18_classes

loss  the loss launch at B = 1024: softmax_ce_kernel at 10 classes beside softmax_ce_wide_kernel (with its
      fold launch) at 100 and 256, one-hot and soft (eps 0.1 + mix rows), with and without the bias
      gradient.  SL_CE_WIDE_ROWS sets the wide kernel's rows per workgroup for the process.
eval  sl_eval_accum at 10 classes beside sl_eval_accum_wide at 100 and 256, at 1,024 and 65,536 rows.
fc    the FC layer's forward, weight-gradient and data-gradient launches at B = 1024 for 10, 100 and 256
      classes, at the dlogits stride the engine uses.
step  the captured ResNet-18 step at B = 1024 with 10 and with 100 classes, interleaved.

The method of scripts/aug_probe.py and scripts/eval_probe.py: device events around a run of launches (or
graph replays), the variants interleaved round by round, microseconds per launch with minimum, median and
maximum over the rounds.  Each prints one JSON line and writes it to <out>/classes_probe_<what>[_<tag>].json.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
B = 1024


def _summary(v, digits=3):
    return {"us_runs": [round(t, digits) for t in v], "us_min": round(min(v), digits),
            "us_max": round(max(v), digits), "us_median": round(statistics.median(v), digits)}


def _interleave(fns: dict, rounds: int, launches: int) -> dict:
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            b.synchronize()
            us[name].append(1e3 * a.elapsed_time(b) / launches)
    return {name: _summary(v) for name, v in us.items()}


def loss(args) -> dict:
    from serverless_learn_amd.ops import cnn as K

    fns = {}
    keep = []
    for ncls in (10, 100, 256):
        g = torch.Generator().manual_seed(ncls)
        z = (torch.randn(B, ncls, generator=g) * 3).to(DEV)
        lab = torch.randint(0, ncls, (B,), generator=g, dtype=torch.uint8).to(DEV)
        mix = torch.zeros(B, 8, dtype=torch.int32)
        mix[:, 0] = (torch.arange(B) + 5) % B
        mix[:, 1], mix[:, 2], mix[:, 3] = (torch.arange(B) * 7) % 257, 256, 1
        mix = mix.to(DEV)
        ld = K.logit_ld(ncls)
        lo, co = torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
        dz = torch.zeros(B, ld, dtype=torch.bfloat16, device=DEV)
        db = torch.zeros(ncls, device=DEV)
        ws = K.softmax_ce_wide_ws(B, ncls, DEV)
        kw = {} if ws is None else dict(ws=ws)
        keep.append((z, lab, mix, lo, co, dz, db, ws))
        fns[f"{ncls}/one_hot"] = lambda z=z, lab=lab, lo=lo, co=co, dz=dz, db=db, kw=kw: K.softmax_ce(
            z, lab, lo, co, dz, db, 1.0 / B, **kw)
        fns[f"{ncls}/one_hot_no_dbias"] = lambda z=z, lab=lab, lo=lo, co=co, dz=dz, kw=kw: K.softmax_ce(
            z, lab, lo, co, dz, None, 1.0 / B, **kw)
        fns[f"{ncls}/soft_mix"] = lambda z=z, lab=lab, lo=lo, co=co, dz=dz, db=db, mix=mix, kw=kw: K.softmax_ce_soft(
            z, lab, lo, co, dz, db, 1.0 / B, mix=mix, eps=0.1, **kw)
    res = {"what": "loss", "batch": B, "rows_per_workgroup": os.environ.get("SL_CE_WIDE_ROWS", "default (16)"),
           "launches": args.launches, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    res.update(_interleave(fns, args.rounds, args.launches))
    return res


def evalk(args) -> dict:
    from serverless_learn_amd.ops import evalmetrics as E

    res = {"what": "eval", "launches": args.launches, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    for rows in (1024, 65536):
        fns, keep = {}, []
        for ncls in (10, 100, 256):
            g = torch.Generator().manual_seed(rows + ncls)
            z = torch.randn(rows, ncls, generator=g).to(DEV)
            lab = torch.randint(0, ncls, (rows,), generator=g).to(torch.uint8).to(DEV)
            lo = torch.rand(rows, generator=g).to(DEV)
            wide = ncls > E.MAX_CLASSES
            acc = E.new_acc_wide(DEV, ncls) if wide else E.new_acc(DEV)
            fn = E.eval_accum_wide if wide else E.eval_accum
            keep.append((z, lab, lo, acc))
            fns[str(ncls)] = lambda fn=fn, z=z, lab=lab, lo=lo, acc=acc, ncls=ncls: fn(z, lab, lo, rows, ncls, 5, acc)
        res[str(rows)] = _interleave(fns, args.rounds, args.launches)
    return res


def fc(args) -> dict:
    from serverless_learn_amd.ops import cnn as K

    fns, keep = {}, []
    for ncls in (10, 100, 256):
        g = torch.Generator().manual_seed(ncls)
        ld = K.logit_ld(ncls)
        feat = torch.randn(B, 1, 1, 512, generator=g).to(torch.bfloat16).to(DEV)
        w = (torch.randn(ncls * 512, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
        bias = torch.zeros(ncls, device=DEV)
        logits = torch.zeros(B, ncls, device=DEV)
        dl = torch.zeros(B, 1, 1, ld, dtype=torch.bfloat16)
        dl[..., :ncls] = torch.randn(B, 1, 1, ncls, generator=g).to(torch.bfloat16) * 0.01
        dl = dl.to(DEV)
        wt = torch.zeros(512 * ld, dtype=torch.bfloat16, device=DEV)
        K.WeightTransposer([(w, wt, ncls, 1, 512, ld)], DEV)()
        gw = torch.zeros(ncls * 512, device=DEV)
        dfeat = torch.zeros(B, 1, 1, 512, dtype=torch.bfloat16, device=DEV)
        ws = K.WgradWorkspace(DEV)
        K.conv_wgrad(feat, dl, ncls, 1, 1, 0, gw, ws=ws)  # sizes the slab
        ws.grow()
        keep.append((feat, w, bias, logits, dl, wt, gw, dfeat, ws))
        fns[f"{ncls}/fwd"] = lambda feat=feat, w=w, ncls=ncls, logits=logits, bias=bias: K.conv_fwd(
            feat, w, ncls, 1, 1, 0, yf=logits, bias=bias)
        fns[f"{ncls}/wgrad"] = lambda feat=feat, dl=dl, ncls=ncls, gw=gw, ws=ws: K.conv_wgrad(
            feat, dl, ncls, 1, 1, 0, gw, ws=ws)
        fns[f"{ncls}/dgrad"] = lambda dl=dl, wt=wt, dfeat=dfeat: K.conv_dgrad(dl, wt, 512, 1, 1, 0, dfeat)
    res = {"what": "fc", "batch": B, "launches": args.launches, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0)}
    res.update(_interleave(fns, args.rounds, args.launches))
    return res


def step(args) -> dict:
    from serverless_learn_amd.data.device_synth import synth_on_device
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    fns, keep = {}, []
    for ncls in args.classes:
        kind = "cifar100" if ncls > 10 else "cifar"
        x, y = synth_on_device(kind, 4 * B, seed=0, device=DEV)
        kw = {} if ncls == 10 else dict(classes=ncls)
        tr = FusedResNetTrainer(batch=B, device=DEV, seed=0, **kw)
        tr.load_shard(x.view(-1, 32, 32, 3), y)
        tr.capture()
        keep.append(tr)
        fns[str(ncls)] = tr.step
    res = {"what": "step", "batch": B, "launches": args.launches, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0)}
    res.update(_interleave(fns, args.rounds, args.launches))
    res["loss"] = {str(tr.spec.classes): tr.stats().loss for tr in keep}
    for tr in keep:
        tr.drop_graphs()
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("what", choices=["loss", "eval", "fc", "step"])
    ap.add_argument("--out", default="")
    ap.add_argument("--tag", default="")
    ap.add_argument("--launches", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--classes", type=int, nargs="+", default=[10, 100])
    args = ap.parse_args()
    args.launches = args.launches or (30 if args.what == "step" else 200)
    res = {"loss": loss, "eval": evalk, "fc": fc, "step": step}[args.what](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        name = f"classes_probe_{args.what}" + (f"_{args.tag}" if args.tag else "") + ".json"
        with open(os.path.join(args.out, name), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
