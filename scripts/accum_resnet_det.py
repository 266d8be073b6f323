#!/usr/bin/env python3
"""Gradient accumulation in the ResNet engine against its definition, in the deterministic kernel
build (SL_DETERMINISTIC=1: a process loads one kernel library, so tests/test_accum_gpu.py runs this
as a child).  ResNet-18, CIFAR stem, batch 32, accum_steps K = 2.  Prints one JSON line.

twin      an accumulating trainer's step at cursor t against a twin with the same weights,
          accum_steps 1 and world_size K (the same gradient scale): the twin's compute_grads() at
          cursors t and t + 1, summed in fp32 on the device, must equal the trainer's grad bit for
          bit; the twin's own update launch on that sum must give the same params / mom; the
          BatchNorm running statistics must equal the twin's after its two forwards.  A recording
          bucket hook (bucket_bytes small enough for several buckets) must be called during the
          last micro-batch only, with slices that tile the flat vector and already hold the sum.
aug       the same equality with shuffle, crop-flip and mixup on and no bucket hook (one
          whole-vector fold); aug_out / mix_out after the step are the twin's at cursor t + 1.
resume    two accumulated steps (AdamW), save through the checkpoint byte format, restore into a
          fresh trainer with another seed, two more steps in both: bit-identical to four straight
          steps.
resume_aug  the same with shuffle and crop-flip on.  The seed keys the input pipeline, so the fresh
          trainer shares it and starts from other weights instead.

Usage: SL_DETERMINISTIC=1 python scripts/accum_resnet_det.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from serverless_learn_amd.ckpt import format as ckfmt
from serverless_learn_amd.data.synthetic import make_cifar_like
from serverless_learn_amd.models.resnet import init_params, resnet18_spec
from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer
from serverless_learn_amd.ops import cnn as K

B, KA, DEV = 32, 2, "cuda:0"
x, y = make_cifar_like(6 * B, seed=5)
x, y = torch.from_numpy(x), torch.from_numpy(y)


def trainer(seed=2, **kw):
    tr = FusedResNetTrainer(batch=B, device=DEV, seed=seed, **kw)
    tr.load_shard(x, y)
    return tr


def same_stats(a, b) -> bool:
    return all(torch.equal(rm, b.running_stats()[name][0]) and torch.equal(rv, b.running_stats()[name][1])
               for name, (rm, rv) in a.running_stats().items())


def twin_case(hooked: bool, t0: int, **kw) -> dict:
    acc = trainer(accum_steps=KA, **kw)
    twin = trainer(world_size=KA, **kw)
    for tr in (acc, twin):
        tr.cursor.fill_(t0)
    rec = []
    if hooked:
        acc.bucket_bytes = 8 << 20

        def hook(view):
            lo = (view.data_ptr() - acc.grad.data_ptr()) // 4
            rec.append((lo, lo + view.numel(), view.clone(), int(acc.cursor.item())))

        acc.bucket_hook = hook
    res = {"grad_scale_equal": acc.grad_scale == twin.grad_scale, "samples_per_step": acc.samples_per_step}
    acc.step()
    parts, losses, corrects = [], [], []
    for i in range(KA):
        parts.append(twin.compute_grads().clone())
        losses.append(twin.loss.clone())
        corrects.append(twin.correct.clone())
        if i < KA - 1:
            K.cursor_bump(twin.cursor)
    total = parts[0]
    for g in parts[1:]:
        total = total + g  # ((g_0 + g_1) + ...), fp32 on the device
    res["grad_identical"] = bool(torch.equal(acc.grad, total))
    res["grad_differs_from_last_micro"] = not bool(torch.equal(acc.grad, parts[-1]))
    res["running_stats_identical"] = same_stats(acc, twin)
    if acc.aug_out is not None:
        res["aug_out_identical"] = bool(torch.equal(acc.aug_out, twin.aug_out))
    if acc.mix_out is not None:
        res["mix_out_identical"] = bool(torch.equal(acc.mix_out, twin.mix_out))
    st = acc.stats()
    lsum = float((losses[0] + losses[1]).sum())
    res["stats_n"] = st.n
    res["loss_identical"] = st.loss == lsum / (KA * B)
    res["accuracy_identical"] = st.accuracy == float((corrects[0] + corrects[1]).sum()) / (KA * B)
    # the twin's unchanged update launch on the sum
    twin.grad.copy_(total)
    twin._update()
    torch.cuda.synchronize()
    res["params_identical"] = bool(torch.equal(acc.params, twin.params))
    res["mom_identical"] = bool(torch.equal(acc.mom, twin.mom))
    res["shadow_identical"] = bool(torch.equal(acc.shadow, twin.shadow))
    res["cursor"] = int(acc.cursor.item()) - t0
    res["finite"] = bool(torch.isfinite(acc.params).all())
    if hooked:
        spans = sorted((lo, hi) for lo, hi, _, _ in rec)
        res["buckets"] = len(rec)
        res["hook_cursors"] = sorted({c - t0 for _, _, _, c in rec})  # KA - 1: during the last micro-batch
        res["buckets_tile"] = (spans[0][0] == 0 and spans[-1][1] == acc.n_params
                               and all(a[1] == b[0] for a, b in zip(spans, spans[1:])))
        res["buckets_hold_sum"] = all(bool(torch.equal(v, total[lo:hi])) for lo, hi, v, _ in rec)
        res["bucket_offsets_mod4"] = sorted({lo % 4 for lo, _, _, _ in rec})
    return res


def resume_case(fresh: dict, **pipeline) -> dict:
    kw = dict(accum_steps=KA, optimizer="adamw", lr=1e-3, weight_decay=1e-2, **pipeline)
    a = trainer(**kw)
    for _ in range(2):
        a.step()
    n = a.n_params
    buf = ckfmt.encode(a.get_flat().cpu().numpy(), {"model": a.model_name, "step": 2}, a.mom[:n].cpu().numpy(),
                       a.state_extra())
    keys = sorted(a.state_extra())
    meta, params, mom, extra = ckfmt.decode_full(buf)
    b = trainer(**fresh, **kw)
    differs_before = not bool(torch.equal(a.params, b.params))
    b.set_flat(torch.from_numpy(params))
    b.mom[:n].copy_(torch.from_numpy(mom))
    b.load_state_extra(extra)
    for _ in range(2):
        a.step()
        b.step()
    torch.cuda.synchronize()
    return {"fresh_trainer_differs": differs_before,
            "params_identical": bool(torch.equal(a.params, b.params)), "mom_identical": bool(torch.equal(a.mom, b.mom)),
            "v_identical": bool(torch.equal(a.v, b.v)), "running_stats_identical": same_stats(a, b),
            "cursor": [int(a.cursor.item()), int(b.cursor.item())],
            "opt_step": [int(a.opt_step.item()), int(b.opt_step.item())],
            "nothing_new_checkpointed": keys == sorted(trainer(**dict(kw, accum_steps=1)).state_extra()),
            "finite": bool(torch.isfinite(a.params).all())}


out = {"deterministic_build": K.deterministic(),
       "twin": twin_case(True, 1),
       "aug": twin_case(False, 2, shuffle=True, augment="crop-flip", mixup_alpha=0.4),
       "resume": resume_case(dict(seed=7)),
       "resume_aug": resume_case(dict(flat=init_params(resnet18_spec("cifar", 10, None), 7)), shuffle=True,
                                 augment="crop-flip")}
print(json.dumps(out))
