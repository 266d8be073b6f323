"""Exact checks of the per-class weight decay (ops/optim.py decay groups): a grouped update must
equal, element by element and bit for bit, the ungrouped update run with the decay of the
element's class.  The yardstick is the existing ungrouped kernel, so no tolerance is involved.

Used in process by tests/test_decay_groups_gpu.py (the shipped kernel build) and by
scripts/decay_groups_det.py (the deterministic build: a process loads one kernel library).
"""
from __future__ import annotations

import itertools

import numpy as np
import torch

from ..ops import optim as O

FLAT_SIZES = (64, 1000, 4099)  # one block; a scalar tail; several chunks per thread with a tail
FLAT_DECAYS = (0.5, 0.25, 0.0)  # weight, norm, bias: large, so a wrong class moves many bits


def select_by_class(cls, n: int, per_class: list) -> torch.Tensor:
    """Element i of ``per_class[class of i]`` (three tensors of n elements)."""
    per = torch.as_tensor(np.asarray(cls)).long().repeat_interleave(O.DECAY_BLOCK)[:n].to(per_class[0].device)
    out = per_class[0].clone()
    for c in (1, 2):
        out[per == c] = per_class[c][per == c]
    return out


def flat_case(device, n: int, adamw: bool, table: bool, shadow: bool, step0: int) -> list:
    """One grouped flat launch against three ungrouped launches on clones; the names of the
    tensors that differ (empty: exact)."""
    gen = torch.Generator().manual_seed(n * 8 + adamw * 4 + table * 2 + shadow)
    rnd = lambda scale: ((torch.rand(n, generator=gen) * 2 - 1) * scale).to(device)  # noqa: E731
    w0, g, m0 = rnd(0.5), rnd(0.1), rnd(0.1)
    v0 = rnd(0.01).abs() if adamw else None
    cls = torch.randint(0, 3, ((n + O.DECAY_BLOCK - 1) // O.DECAY_BLOCK,), generator=gen).to(torch.uint8)
    kw = dict(lr_schedule="cosine", lr_warmup_steps=2, lr_decay_steps=8) if table or not adamw else {}
    spec = lambda wd, **grp: O.OptSpec(lr=0.05, momentum=0.9, weight_decay=wd,  # noqa: E731
                                       optimizer="adamw" if adamw else "sgd", **kw, **grp)
    grouped = spec(FLAT_DECAYS[0], norm_weight_decay=FLAT_DECAYS[1], bias_weight_decay=FLAT_DECAYS[2])
    # the ungrouped scheduled-SGD entry point has no scalar-lr form: without a table it gets a
    # one-entry table that holds the scalar
    tab = torch.from_numpy(grouped.lr_table()).to(device) if table else None
    tab1 = tab if table else torch.full((1,), grouped.lr, dtype=torch.float32, device=device)
    step = torch.full((1,), step0, dtype=torch.int32, device=device)
    gscale = 0.37

    def run(s: O.OptSpec, groups: bool) -> dict:
        w, m = w0.clone(), m0.clone()
        v = v0.clone() if adamw else None
        sh = torch.zeros(n, dtype=torch.bfloat16, device=device) if shadow else None
        if adamw and groups:
            O.adamw_flat_groups(w, g, m, v, step, s, cls.to(device), tab, shadow=sh, grad_scale=gscale)
        elif adamw:
            O.adamw_flat(w, g, m, v, step, s, tab, shadow=sh, grad_scale=gscale)
        elif groups:
            O.sgd_flat_lr_groups(w, g, m, step, tab, cls.to(device), s.decays(), lr=s.lr, momentum=s.momentum,
                                 shadow=sh, grad_scale=gscale)
        else:
            O.sgd_flat_lr(w, g, m, step, tab1, s.momentum, s.weight_decay, shadow=sh, grad_scale=gscale)
        return {"w": w, "mom": m, "v": v, "shadow": sh}

    got = run(grouped, True)
    refs = [run(spec(d), False) for d in FLAT_DECAYS]
    torch.cuda.synchronize()
    bad = []
    for name, t in got.items():
        if t is None:
            continue
        want = select_by_class(cls, n, [r[name] for r in refs])
        if not torch.equal(t, want):
            bad.append(f"{name}: {int((t != want).sum())} of {n} differ")
    # the three references must differ from one another, or the selection shows nothing
    assert not torch.equal(refs[0]["w"], refs[1]["w"]) and not torch.equal(refs[1]["w"], refs[2]["w"])
    return bad


def flat_cases():
    """(n, adamw, table, shadow, step0) of every flat case."""
    return list(itertools.product(FLAT_SIZES, (True, False), (True, False), (True, False), (0, 5)))


def flat_failures(device) -> dict:
    """Every flat case that is not exact: {case: what differs}."""
    out = {}
    for case in flat_cases():
        bad = flat_case(device, *case)
        if bad:
            out[str(case)] = bad
    return out
