#!/usr/bin/env python3
"""Two-rank check of the xGMI update kernel under AdamW (mlp_fused.hip mlp_opt_update_kernel).

Launched by tests/test_optim_gpu.py as
``torchrun --nproc-per-node 2 scripts/optim_xgmi_check.py --same-device`` (the ranks share the
GPU, as in scripts/xgmi_check.py).  The ranks train on different halves of one shard with AdamW
for 4 steps, first with the one-shot exchange, then with the two-shot one.  Per protocol:

1. the replicas stay bit-identical (parameters, both moments, optimizer step);
2. they equal a second trainer in the same process that takes the update-from-gradient path,
   its hook summing the ranks' reduced gradients in rank order through host memory;
3. no barrier timed out.
Prints ``OPTIM_XGMI_OK rank=R`` on success; any failure raises (non-zero exit).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.distributed as dist

STEPS = 4
ADAMW = dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2)


def main() -> int:
    same = "--same-device" in sys.argv
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0 if same else int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    from serverless_learn_amd.data.synthetic import make_mnist_like
    from serverless_learn_amd.models.mlp import FusedMLPTrainer
    from serverless_learn_amd.parallel.xgmi import XgmiExchange, dist_collectives

    B = 128
    x, y = make_mnist_like(2 * B * world, seed=3)
    xt = torch.from_numpy(x)[rank * 2 * B:(rank + 1) * 2 * B]  # this rank's half: two batches
    yt = torch.from_numpy(y)[rank * 2 * B:(rank + 1) * 2 * B]

    def host_allreduce(g):
        """All-reduce through host memory, summing in rank order as the kernel does."""
        parts = [torch.empty(g.numel()) for _ in range(world)]
        dist.all_gather(parts, g.cpu())
        acc = parts[0].clone()
        for q in range(1, world):
            acc += parts[q]
        g.copy_(acc.to(g.device))

    for two in (False, True):
        a = FusedMLPTrainer(batch=B, device=dev, world_size=world, seed=0, **ADAMW)
        b = FusedMLPTrainer(batch=B, device=dev, world_size=world, seed=0, **ADAMW)
        a.load_shard(xt, yt)
        b.load_shard(xt, yt)
        b.allreduce = host_allreduce
        xa = XgmiExchange(a.n_pad, rank, world, dev, *dist_collectives(), two_shot=two)
        a.enable_xgmi(xa)
        for step in range(STEPS):
            b.step()
            a.step()
            torch.cuda.synchronize()
            assert not xa.error(), f"xgmi barrier timed out at step {step} (two_shot={two})"
        for name in ("params", "mom", "v", "opt_step", "cursor", "w1h", "w2h", "r1p"):
            ta, tb = getattr(a, name), getattr(b, name)
            assert torch.equal(ta, tb), f"two_shot={two}: {name} differs from the host all-reduce run " \
                                        f"({int((ta != tb).sum())} elements)"
            mine = ta.detach().cpu()
            ref = mine.clone()
            dist.broadcast(ref, 0)
            assert torch.equal(mine, ref), f"two_shot={two}: replicas diverged in {name}"
        assert int(a.opt_step.item()) == STEPS and int(a.opt_ticket.item()) == 0
        dist.barrier()  # every rank's kernels are done with every peer's buffer before anyone unmaps
        torch.cuda.synchronize()
        xa.close()
    print(f"OPTIM_XGMI_OK rank={rank} steps={STEPS} loss={a.stats().loss:.4f}", flush=True)
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
