#!/usr/bin/env python3
"""Diagnostic: the MLP weight gradient's main loop per tile kind, inside bench.py's 20-step graph.

Per tile kind (dW1 full tiles, dW1's 16-column tail tile, dW2 tiles): s_memtime ticks per 64-row
stage of the main loop and, with a kernel library built with -DSL_WG_WAITSTAMP (8 stamps per
workgroup; pass it through SL_KERNELS_SO), the share of those ticks wave 0 spent in the steps'
wg_vmcnt (its own LDS-DMA pieces) and s_barrier (everyone's).  Also the launch's span on the
chip-wide 100 MHz clock and the step time from events.  The stamps are those of the last step of
the last replay.
Usage: [SL_KERNELS_SO=build.so] python scripts/wgrad_stage_stamps.py [wide: 1|0]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from serverless_learn_amd.data.synthetic import make_mnist_like
from serverless_learn_amd.models.mlp import FusedMLPTrainer
from serverless_learn_amd.ops import _native

B, UNROLL = 65536, 20
lib = _native.lib()
if len(sys.argv) > 1 and hasattr(lib, "sl_mlp_set_wg_wide"):  # (an older build has only the 256 x 128 loop)
    _native.call("sl_mlp_set_wg_wide", int(sys.argv[1]))
NST = int(lib.sl_mlp_wg_stamps()) if hasattr(lib, "sl_mlp_wg_stamps") else 6
x, y = make_mnist_like(B * 4, seed=0)
tr = FusedMLPTrainer(batch=B, device="cuda:0")
tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
nwg = 9 * tr.slices
st = torch.zeros(nwg * NST, dtype=torch.int64, device="cuda:0")
_native.call("sl_mlp_set_wg_stamps", st.data_ptr())
tr._lc = None; tr._lkey = None
tr.capture(warmup=2, unroll=UNROLL)
_native.call("sl_mlp_set_wg_stamps", None)
for _ in range(5):
    tr.steps(UNROLL)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
reps = 10
e0.record()
for _ in range(reps):
    tr.steps(UNROLL)
e1.record()
torch.cuda.synchronize()
print(f"step (events, {reps} x {UNROLL}-step graph, stamps on): {e0.elapsed_time(e1) * 1000.0 / (reps * UNROLL):.1f} us")

s = st.view(nwg, NST).cpu().double()
assert bool((s[:, 4] > 0).all()), "stamps missing"
total = B // 64
spp = (total + tr.slices - 1) // tr.slices
sl = torch.arange(nwg) // 9
stages = torch.clamp(total - sl * spp, max=spp).double()
tile = torch.arange(nwg) % 9
mhz = float(((s[:, 2] - s[:, 0]) / ((s[:, 5] - s[:, 4]) / 100.0)).median())
print(f"s_memtime ticks per us over a workgroup (median): {mhz:.0f};  slices {tr.slices}, stages per slice {spp}")
for name, sel in (("dW1 full tiles 0-5", tile < 6), ("dW1 tail tile 6", tile == 6), ("dW2 tiles 7-8", tile >= 7)):
    v, n = s[sel], stages[sel]
    loop = v[:, 1] - v[:, 0]
    line = (f"{name:20s} n={int(sel.sum()):3d}  main loop ticks median {float(loop.median()):7.0f} max {float(loop.max()):7.0f}"
            f"  per stage median {float((loop / n).median()):6.0f}  whole WG median {float((v[:, 2] - v[:, 0]).median()):7.0f}")
    if NST >= 8:
        line += (f"  wait share: vmcnt {float((v[:, 6] / loop).median()) * 100:4.1f} %  barrier "
                 f"{float((v[:, 7] / loop).median()) * 100:4.1f} %  both {float(((v[:, 6] + v[:, 7]) / loop).median()) * 100:4.1f} %")
    print(line)
print(f"wgrad span (first start -> last end, 100 MHz clock): {float(s[:, 5].max() - s[:, 4].min()) * 0.01:.2f} us;  "
      f"median workgroup {float((s[:, 5] - s[:, 4]).median()) * 0.01:.2f} us")
