#!/usr/bin/env python3
"""In-process interleaved A/B of kernel LIBRARIES (two or more builds of libslkernels.so).

The package loads its one library RTLD_GLOBAL, which keeps a second build from coexisting
(scripts/ab_mlp_inproc.py, scripts/ab_env.sh).  Here each build is loaded RTLD_LOCAL |
RTLD_DEEPBIND, one trainer per build captures bench.py's 20-step graph while that build is the
package's current library, and the arms then alternate rounds of pure graph replays: no process
or box difference between the arms.  Prints per-arm medians, every round, and whether the arms'
parameters ended bit-identical.
A path may end in @rows, @wgrad or @off: only that launch (or neither) reads X from the tiled
shard, the other from the row-major one (the per-consumer arms of profiles/r11_xtile).
Usage: python scripts/ab_mlp_libs.py ROUNDS STEPS name=/path/to/build.so name2=/path/to/other.so[@rows] ..."""
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from serverless_learn_amd.data.synthetic import make_mnist_like
from serverless_learn_amd.models.mlp import FusedMLPTrainer
from serverless_learn_amd.ops import _native

R, N, B = int(sys.argv[1]), int(sys.argv[2]), 65536
arms = [a.split("=", 1) for a in sys.argv[3:]]
x, y = make_mnist_like(B * 4, seed=0)
xs, ys = torch.from_numpy(x), torch.from_numpy(y)
trs = {}
for name, path in arms:
    path, _, only = path.partition("@")
    h = ctypes.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    for fn in _native._SIGS:
        if hasattr(h, fn):
            _native._bind(h, fn)
    _native._lib = h
    print(name, "sl_mlp_rows at", hex(ctypes.cast(h.sl_mlp_rows, ctypes.c_void_p).value), file=sys.stderr)
    tr = FusedMLPTrainer(batch=B, device="cuda:0")
    tr.load_shard(xs, ys)
    if only:
        xt, tr.xt = tr.xt, None
        plain = dict(tr._launches())
        tr.xt = xt
        lc = tr._launches()  # cached under the tiled key: the swapped entries stay
        for k in ("rows", "wgrad"):
            if k != only:
                lc[k] = plain[k]
        print(name, {k: lc[k].entry for k in ("rows", "wgrad")}, file=sys.stderr)
    tr.capture(warmup=2, unroll=20)
    tr.steps(200)
    torch.cuda.synchronize()
    trs[name] = tr
for _ in range(4):  # un-timed interleaved rounds: the first timed round runs ~1 us high in every arm
    for tr in trs.values():
        tr.steps(N)
        torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t = {name: [] for name in trs}
for r in range(R):
    for name, tr in trs.items():
        e0.record()
        tr.steps(N)
        e1.record()
        torch.cuda.synchronize()
        t[name].append(round(e0.elapsed_time(e1) / N * 1e3, 2))
ref = next(iter(trs.values())).get_flat()
for name, tr in trs.items():
    print("ARM", name, json.dumps({"median": statistics.median(t[name]), "min": min(t[name]), "max": max(t[name]),
                                   "all": t[name], "params_equal_first_arm": bool(torch.equal(tr.get_flat(), ref)),
                                   "loss": tr.stats().loss}))
