"""Exact, element-wise checks of the fused MLP step (csrc/kernels/mlp_fused.hip): the rows kernel in
its training and evaluation forms, the weight gradient with its slab reduce, and the three forms of
the momentum-SGD update with every shadow they write.

The operands make every quantity of the step exactly representable where the kernels store it.
``xa`` / ``xb`` / ``grad_scale`` / ``dh1_scale`` are launch arguments, so a case passes powers of
two: the normalised pixels ``xa u + xb`` are then the integers -1 .. 2, W1 and W2 are in {-1, 0, 1},
the biases are integers, and H1 / H2 are integers of at most 8 significant bits (bf16).  W3 and b3
are multiples of 128 with groups of classes sharing one row: two logits are equal or at least 128
apart, ``exp(-128)`` is 0 in fp32, so a row with ``m`` maxima (m a power of two) has probabilities
exactly 1/m or 0 and dZ is a multiple of grad_scale / 8.  The backward products are multiples of
16 grad_scale with a few significant bits, every GEMM's sum of absolute terms stays below 2^24 of
its unit (any summation order and any split-K give the same bits), and with lr = 2^-2, mu = 2^-1,
wd = 2^-4 and an integer momentum every intermediate of the update is an fp32 value.  A kernel's
output must therefore EQUAL a float64 reference, element for element (``torch.equal``); only the
per-row loss (a logarithm) keeps a bound, derived in :func:`reference`.  The conditions are
asserted on the reference alone (:func:`check_case_bounds`) before any kernel output is looked at.

This module holds the case table (:data:`CASES`), the seeded generator (:func:`operands`), the
float64 reference (:func:`reference`), the comparator (:func:`compare`) and the drivers that run
one case through the launchers (:func:`run_case`, :func:`run_update`).  Everything but the drivers
runs on the CPU.  Used by tests/test_mlp_exact.py, tests/test_mlp_exact_gpu.py and
scripts/mlp_exact_check.py.
"""
from __future__ import annotations

import functools
import math
import os
from dataclasses import dataclass

import torch

from ..models import mlp as M

F32_EXACT = float(2 ** 24)  # sums of multiples of q whose absolute terms stay below 2^24 q are exact in fp32
W3P_N = M.CLASSES * M.HIDDEN + M.CLASSES  # [dW3 | db3] of a partial row (mlp_fused.hip)
W3P_DB1 = 2576
W3P_DB2 = W3P_DB1 + M.HIDDEN
KS1, KS2 = M.D_IN_PAD // 32, M.HIDDEN // 32  # 32-deep k-steps per fragment row of the shadows
LR, MU, WD = 2.0 ** -2, 2.0 ** -1, 2.0 ** -4
LOGIT_GAP = 128.0
MOM_BIG = 8192  # |preset momentum| of W1 / W2 entries


# ---------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One batch shape and the launcher paths it is in the table for.

    bm: the rows tile the launcher must pick (force_bm: through sl_mlp_set_rows_bm).  slices:
    (requested, effective) split-K slice counts of the weight gradient, requested None = the
    library's default.  shard / cursor: rows of the resident shard and the device cursor (the batch
    is rows cursor % n_batches * batch ...).  x_step / xa / xb: pixels are x_step * {0..3} and
    xa u + xb = u / x_step - 1.  ties: groups of classes with one W3 row and bias."""
    name: str
    batch: int
    bm: int
    slices: tuple
    force_bm: int = 0
    shard: int = 0
    cursor: int = 0
    x_step: int = 1
    ties: tuple = ((0, 1), (2, 3, 4, 5))
    update: bool = False
    why: str = ""

    @property
    def xa(self) -> float:
        return 1.0 / self.x_step

    @property
    def xb(self) -> float:
        return -1.0

    @property
    def grad_scale(self) -> float:
        """The power of two nearest 1 / batch."""
        return 2.0 ** -round(math.log2(self.batch))

    @property
    def dh1_scale(self) -> float:
        """Stored dH1 (fp16) = dH1 / (128 grad_scale): multiples of 1/8."""
        return 1.0 / (128.0 * self.grad_scale)

    @property
    def rows(self) -> int:
        return self.shard or self.batch

    @property
    def seed(self) -> int:
        return [c.name for c in CASES].index(self.name)


CASES = [
    Case("S64", 64, 64, ((None, 1),), update=True, why="one workgroup, one stage"),
    Case("S128", 128, 128, ((None, 2),), update=True, why="one 128-row workgroup"),
    Case("S128h", 128, 64, ((None, 2),), force_bm=64, why="two 64-row workgroups, two partial rows"),
    Case("S320", 320, 64, ((3, 3),), why="short last slice (2 + 2 + 1 stages)"),
    Case("S384", 384, 128, ((4, 3), (None, 6)), update=True,
         why="multi-stage slices; more slices than the reduce's threads per group"),
    Case("S1792", 1792, 128, ((None, 28),), why="the benchmark's slice count, all four slice partitions of the reduce"),
    Case("C256", 128, 128, ((None, 2),), shard=256, cursor=1, why="the device cursor offset in rows and wgrad"),
    Case("P128", 128, 128, ((None, 2),), x_step=64, why="bytes with the high bit set, xa != 1"),
    Case("T128", 128, 128, ((None, 2),), ties=((0, 1, 2, 3, 4, 5, 6, 7),), why="m = 8"),
]
CASES_BY_NAME = {c.name: c for c in CASES}
assert len(CASES_BY_NAME) == len(CASES)
UPDATE_CASES = [c for c in CASES if c.update]
# run by scripts/mlp_exact_check.py in a fresh process
SUBSETS = {"det": ["S64", "S128", "S320"]}


# ---------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------
def _tern(shape, density, g):
    s = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (s * (torch.rand(shape, generator=g) < density)).double()


def _pixels(n, step, g):
    v = torch.randint(1, 4, (n, M.D_IN), generator=g) * step
    return (v * (torch.rand(n, M.D_IN, generator=g) < 0.125)).to(torch.uint8)


def _forward(case, w, x_u8):
    """float64 forward of rows x_u8: p1, h1, p2, h2, z."""
    xn = x_u8.double() * case.xa + case.xb
    p1 = xn @ w["fc1.weight"].t() + w["fc1.bias"]
    h1 = torch.relu(p1)
    p2 = h1 @ w["fc2.weight"].t() + w["fc2.bias"]
    h2 = torch.relu(p2)
    z = h2 @ w["fc3.weight"].t() + w["fc3.bias"]
    return p1, h1, p2, h2, z


def _maxima(z):
    """Per row: the maximum, the mask of the classes that reach it, their count, and the gap to
    the largest other logit (inf when all are maxima)."""
    mx = z.max(1, keepdim=True).values
    ismax = z == mx
    rest = torch.where(ismax, torch.full_like(z, -math.inf), z).max(1).values
    return mx[:, 0], ismax, ismax.sum(1), mx[:, 0] - rest


def _bf16_exact(t):
    return torch.equal(t.to(torch.bfloat16).double(), t)


@functools.lru_cache(maxsize=None)
def operands(case: Case) -> dict:
    """The case's inputs, seeded by its place in the table: x u8 [rows, 784] and y u8 [rows] (the
    whole shard), flat fp32 parameters, mom0 (an integer-valued momentum), and the launch scalars
    xa, xb, grad_scale, dh1_scale, lr, mu, wd.  Rows whose maxima are not 1, 2, 4 or 8 (or that
    leave bf16's integers) are drawn again; a column of X that is zero over the batch gets one
    pixel.  Cached: never modify the result."""
    g = torch.Generator().manual_seed(4000 + case.seed)
    w1 = _tern((M.HIDDEN, M.D_IN), 0.125, g)
    # b1 cancels the row sum the normalisation's -1 brings in: p1 = W1 u + small, balanced around 0
    b1 = w1.sum(1) + torch.randint(-2, 3, (M.HIDDEN,), generator=g).double()
    w2 = _tern((M.HIDDEN, M.HIDDEN), 0.125, g)
    rep = list(range(M.CLASSES))
    for grp in case.ties:
        for c in grp:
            rep[c] = grp[0]
    x = _pixels(case.rows, case.x_step, g)
    # b2 likewise cancels each feature's mean over the rows (H1 >= 0: a W2 row with more -1 than +1
    # would never switch on, and its columns of dH2 and dW2 would be zero)
    mu1 = torch.relu((x.double() * case.xa + case.xb) @ w1.t() + b1).mean(0)
    b2 = torch.randint(-2, 3, (M.HIDDEN,), generator=g).double() - torch.round(w2 @ mu1)
    w = {"fc1.weight": w1, "fc1.bias": b1, "fc2.weight": w2, "fc2.bias": b2,
         "fc3.weight": torch.zeros(M.CLASSES, M.HIDDEN, dtype=torch.float64),
         "fc3.bias": torch.zeros(M.CLASSES, dtype=torch.float64)}
    # W3: one row in {-128, 0, 128} per group of tied classes.  H2 >= 0 gives every row a mean logit
    # of its own, and the class with the largest would win every sample: entries are changed, the
    # most effective first, until each row's mean is within 8 * 128 of zero.  Then no column is the
    # same in every row (its dH2 would be zero whatever the label).
    mu2 = _forward(case, w, x)[3].mean(0)
    distinct = sorted(set(rep))
    w3d = _tern((len(distinct), M.HIDDEN), 0.5, g)
    vals = torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64)
    for row in w3d:
        for _ in range(64):
            r = float(row @ mu2)
            if abs(r) <= 8.0:
                break
            cand = (r + (vals[None, :] - row[:, None]) * mu2[:, None]).abs()  # [column][new value]
            j, v = divmod(int(cand.argmin()), 3)
            row[j] = vals[v]
    for j in (w3d == w3d[0]).all(0).nonzero().reshape(-1).tolist():
        w3d[j % len(distinct), j] = 0.0 if w3d[0, j] != 0 else 1.0
    w["fc3.weight"] = (w3d * 128.0)[[distinct.index(r) for r in rep]]
    w["fc3.bias"] = (torch.randint(-1, 2, (M.CLASSES,), generator=g).double() * 128.0)[rep]
    flat = torch.cat([w[name].reshape(-1) for name, _ in M.LAYOUT]).float()
    lo = (case.cursor % (case.rows // case.batch)) * case.batch
    for _ in range(64):
        xb = x[lo:lo + case.batch]
        for col in (xb.sum(0) == 0).nonzero().reshape(-1).tolist():  # (sum of u8 promotes to int64)
            xb[int(torch.randint(0, case.batch, (1,), generator=g)), col] = case.x_step * int(
                torch.randint(1, 4, (1,), generator=g))
        _, h1, _, h2, z = _forward(case, w, x)
        _, _, m, gap = _maxima(z)
        pow2 = (m == 1) | (m == 2) | (m == 4) | (m == 8)
        rep_ok = ((h1.to(torch.bfloat16).double() == h1) & (h2.to(torch.bfloat16).double() == h2)).all(1)
        bad = (~(pow2 & (gap >= LOGIT_GAP) & rep_ok)).nonzero().reshape(-1)
        if bad.numel() == 0 and int((xb.sum(0) == 0).sum()) == 0:
            break
        x[bad] = _pixels(bad.numel(), case.x_step, g)
    else:
        raise AssertionError(f"{case.name}: no admissible rows after 64 rounds")
    # labels, by quota within every batch of the shard (in a random order of its rows): 28 % of the
    # rows have one maximum and that class as their label (dZ identically 0), 45 % a class that is not
    # among the maxima (the only rows with a non-zero dH2: a batch of 64 needs that many for every
    # column of dH2 to see one), the rest one of the maxima
    _, ismax, m, _ = _maxima(z)
    among = torch.multinomial(ismax.double(), 1, generator=g)[:, 0]
    other = torch.multinomial((~ismax).double() + 1e-9, 1, generator=g)[:, 0]  # (all ten tied: any class)
    y = among.clone()
    for b0 in range(0, case.rows, case.batch):
        order = b0 + torch.randperm(case.batch, generator=g)
        single = order[m[order] == 1]
        n_zero, n_not = math.ceil(0.28 * case.batch), math.ceil(0.45 * case.batch)
        assert single.numel() >= n_zero, (case.name, single.numel())
        keep = set(single[:n_zero].tolist())
        rest = [r for r in order.tolist() if r not in keep][:n_not]
        y[rest] = other[rest]
    y = y.to(torch.uint8)
    # integer momentum: large for W1 and W2, so that w - lr (mu m0 + ...) has more significant bits
    # than the fp16 / bf16 shadows keep and the shadow write rounds; small where the gradient is fine-grained
    mom0 = torch.randint(-2, 3, (M.N_PARAMS,), generator=g).float()
    for name, shape, off, n in M.param_layout():
        if name in ("fc1.weight", "fc2.weight"):
            mom0[off:off + n] = torch.randint(-MOM_BIG, MOM_BIG + 1, (n,), generator=g).float()
    return {"x": x, "y": y, "flat": flat, "mom0": mom0, "xa": case.xa, "xb": case.xb,
            "grad_scale": case.grad_scale, "dh1_scale": case.dh1_scale, "lr": LR, "mu": MU, "wd": WD}


# ---------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------
def ulp32(v) -> torch.Tensor:
    """Spacing of fp32 at magnitude v (float64 tensor, v >= 2^-126)."""
    return torch.exp2(torch.floor(torch.log2(v)) - 23.0)


def _sumabs(a, b):
    """Largest sum of absolute terms over the outputs of a @ b."""
    return float((a.abs() @ b.abs()).max())


def _f32_exact(t) -> bool:
    return torch.equal(t.float().double(), t)


def _multiple(t, q) -> bool:
    return torch.equal(torch.round(t / q) * q, t)


def _pow2_unit(t) -> float:
    """The largest power of two (2^-40 .. 2^20) of which every element of t is a multiple."""
    for e in range(20, -41, -1):
        if _multiple(t, 2.0 ** e):
            return 2.0 ** e
    raise AssertionError("no power-of-two unit down to 2^-40")


@functools.lru_cache(maxsize=None)
def reference(case: Case) -> dict:
    """Every quantity of the step for the case's operands, float64, from the definition (plain
    matrix products, ReLU mask p > 0, probabilities ismax / m), plus what proves the comparison
    exact: "maxima", "sumabs" (per GEMM, in its unit q: every term a multiple of q), "shares".
    Cached: never modify the result."""
    o = operands(case)
    w = {k: v.double() for k, v in M.views(o["flat"]).items()}
    lo = (case.cursor % (case.rows // case.batch)) * case.batch
    xu = o["x"][lo:lo + case.batch].double()
    y = o["y"][lo:lo + case.batch].long()
    gs, s1 = case.grad_scale, case.dh1_scale
    p1, h1, p2, h2, z = _forward(case, w, o["x"][lo:lo + case.batch])
    mx, ismax, m, gap = _maxima(z)
    onehot = torch.nn.functional.one_hot(y, M.CLASSES).double()
    dz = (ismax.double() / m[:, None].double() - onehot) * gs
    dh2 = (dz @ w["fc3.weight"]) * (p2 > 0).double()
    dh1 = (dh2 @ w["fc2.weight"]) * (p1 > 0).double()
    dh1s = dh1 * s1
    zl = z.gather(1, y[:, None])[:, 0]
    loss = torch.logsumexp(z, 1) - zl
    # the kernel: lse = mx + __logf(s), loss = lse - z_label.  s = m exactly; the log is within
    # 4 * 2^-22 of ln m (tests/test_mlp_rows_epilogue_gpu.py test_ties_take_the_first_class), the sum
    # mx + log rounds once at a magnitude <= |mx| + 3, the difference once at <= max(|mx|, |z_label|) + 3
    # (both roundings lie below half an ulp there; one ulp covers the two)
    loss_bound = ulp32(torch.maximum(mx.abs(), zl.abs()) + 3.0) + 4 * 2.0 ** -22
    correct = (ismax.double().argmax(1) == y).double()  # the lowest index among the maxima

    slab = dh1s.t() @ (1024.0 + xu)
    db1, db2, db3 = dh1.sum(0), dh2.sum(0), dz.sum(0)
    a, b = M.dw1_coeffs(case.xa, case.xb, s1)
    dw1 = a * slab + b * db1[:, None]
    assert torch.equal(dw1, dh1.t() @ (xu * case.xa + case.xb)), case.name  # the same thing, from the definition
    dw2, dw3 = dh2.t() @ h1, dz.t() @ h2
    grad = torch.cat([dw1.reshape(-1), db1, dw2.reshape(-1), db2, dw3.reshape(-1), db3])

    # the rows kernel's partial rows: one per workgroup of bm rows
    nrow = case.batch // case.bm
    w3p = torch.zeros(nrow, M.W3P_LD, dtype=torch.float64)
    for r in range(nrow):
        sl = slice(r * case.bm, (r + 1) * case.bm)
        w3p[r, :M.CLASSES * M.HIDDEN] = (dz[sl].t() @ h2[sl]).reshape(-1)
        w3p[r, M.CLASSES * M.HIDDEN:W3P_N] = dz[sl].sum(0)
        w3p[r, W3P_DB1:W3P_DB2] = dh1[sl].sum(0)
        w3p[r, W3P_DB2:] = dh2[sl].sum(0)

    # momentum SGD from the preset momentum (torch.optim.SGD semantics, ops/optim.py sgd_update)
    w0, m0 = o["flat"].double(), o["mom0"].double()
    t_wd = WD * w0
    t_d = grad + t_wd
    t_mu = MU * m0
    mom = t_mu + t_d
    t_lr = LR * mom
    params = w0 - t_lr
    nv = M.views(params)
    w1h = nv["fc1.weight"].float().to(torch.float16)
    ref = {
        "h1": h1, "h2": h2, "z": z, "dz": dz, "dh2": dh2, "dh1": dh1, "dh1s": dh1s, "loss": loss,
        "loss_bound": loss_bound, "correct": correct, "w3p": w3p, "grad": grad, "slab": slab,
        "p1": p1, "p2": p2, "m": m, "gap": gap, "ismax": ismax, "y": y, "xu": xu,
        "params": params, "mom": mom, "update_terms": (t_wd, t_d, t_mu, mom, t_lr, params, a * slab, b * db1),
        "w1h": w1h.double(), "w2h": nv["fc2.weight"].float().to(torch.bfloat16).double(),
        "w3h": nv["fc3.weight"].float().to(torch.bfloat16).double(),
        "r1": torch.round(w1h.double() * 2.0 ** 24).long().sum(1),
    }
    # per GEMM: the sum of absolute terms in units of q, the largest power of two that divides every
    # term (the product of the operands' own).  Below 2^24, every partial sum in any order is a
    # multiple of q below 2^24 q: an fp32 value.
    w3u = _pow2_unit(w["fc3.weight"])
    u = ref["units"] = {"dz": _pow2_unit(dz), "dh2": _pow2_unit(dh2), "dh1": _pow2_unit(dh1), "dh1s": _pow2_unit(dh1s)}
    ref["sumabs"] = {
        "layer1": _sumabs(1024.0 + xu, w["fc1.weight"].t()),
        "layer2": _sumabs(h1, w["fc2.weight"].t()),
        "layer3": _sumabs(h2, w["fc3.weight"].t()) / w3u + float(w["fc3.bias"].abs().max()) / w3u,
        "dh2": _sumabs(dz, w["fc3.weight"]) / (u["dz"] * w3u),
        "dh1": _sumabs(dh2, w["fc2.weight"]) / u["dh2"],
        "slab": _sumabs(dh1s.t(), 1024.0 + xu) / u["dh1s"],
        "dw2": _sumabs(dh2.t(), h1) / u["dh2"],
        "dw3": _sumabs(dz.t(), h2) / u["dz"],
        "db1": float(dh1.abs().sum(0).max()) / u["dh1"],
        "db2": float(dh2.abs().sum(0).max()) / u["dh2"],
        "db3": float(dz.abs().sum(0).max()) / u["dz"],
    }
    ref["maxima"] = {
        "h1": float(h1.max()), "h2": float(h2.max()), "z": float(z.abs().max()),
        "dh2": float(dh2.abs().max()) / gs, "dh1": float(dh1.abs().max()) / gs, "dh1s": float(dh1s.abs().max()),
        "dw1": float(dw1.abs().max()), "dw2": float(dw2.abs().max()), "dw3": float(dw3.abs().max()),
        "loss": float(loss.max()), "loss_bound": float(loss_bound.max()),
    }
    among = (ismax & (onehot > 0)).any(1)
    nw2 = nv["fc2.weight"]
    ref["shares"] = {
        **{"m%d" % k: float((m == k).double().mean()) for k in (1, 2, 4, 8)},
        "label_among": float(among.double().mean()), "label_not_among": float((~among).double().mean()),
        "dz_zero": float((dz == 0).all(1).double().mean()),
        "relu1_on": float((p1 > 0).double().mean()), "relu2_on": float((p2 > 0).double().mean()),
        "p1_zero": float((p1 == 0).double().mean()), "p2_zero": float((p2 == 0).double().mean()),
        "dw1_nonzero": float((dw1 != 0).double().mean()), "dw2_nonzero": float((dw2 != 0).double().mean()),
        "w2_rounds": float((nw2.float().to(torch.bfloat16).double() != nw2).double().mean()),
        "w1_rounds": float((w1h.double() != nv["fc1.weight"]).double().mean()),
    }
    return ref


def check_case_bounds(case: Case, ref: dict) -> dict:
    """The conditions that make the comparison exact and not vacuous, asserted on the reference
    alone.  Returns the shares."""
    o = operands(case)
    n, gs = case.name, case.grad_scale
    w = {k: v.double() for k, v in M.views(o["flat"]).items()}
    s = ref["shares"]

    def need(cond, what):
        assert cond, "%s: %s does not hold (%s)" % (n, what, {k: round(v, 4) for k, v in s.items()})

    f16_exact = lambda t: torch.equal(t.float().to(torch.float16).double(), t)  # noqa: E731
    # storage formats
    need(_bf16_exact(ref["h1"]) and _multiple(ref["h1"], 1.0), "H1 integers that survive bf16")
    need(_bf16_exact(ref["h2"]) and _multiple(ref["h2"], 1.0), "H2 integers that survive bf16")
    need(_bf16_exact(ref["dz"] / gs) and _multiple(ref["dz"], gs / 8.0), "dZ / grad_scale eighths that survive bf16")
    need(_bf16_exact(ref["dh2"] / gs), "dH2 / grad_scale survives bf16")
    need(_bf16_exact(ref["dh1"] / gs), "dH1 / grad_scale survives bf16 (the 64-row tile's image)")
    need(f16_exact(ref["dh1s"]), "stored dH1 survives fp16")
    need(f16_exact(w["fc1.weight"]), "W1 survives fp16")
    need(_bf16_exact(w["fc2.weight"]) and _bf16_exact(w["fc3.weight"]), "W2 / W3 survive bf16")
    need(_multiple(w["fc3.weight"], 128.0) and _multiple(w["fc3.bias"], 128.0), "W3 / b3 multiples of 128")
    for key in ("fc1.bias", "fc2.bias", "fc1.weight", "fc2.weight"):
        need(_multiple(w[key], 1.0), key + " integer")
    # layer 1's folded bias b1 + (xb - 1024 xa) R and its scale xa (fma or not: both terms exact)
    fold = w["fc1.bias"] + (case.xb - 1024.0 * case.xa) * w["fc1.weight"].sum(1)
    need(_f32_exact(fold) and _multiple(fold, 1.0) and _multiple(case.xa * (1024.0 + ref["xu"]), 1.0), "layer-1 bias fold")
    # every GEMM: sum of absolute terms below 2^24 units; the fp32 outputs and the update's terms
    for key, v in ref["sumabs"].items():
        need(v < F32_EXACT, "sum of absolute terms of %s = %g below 2^24" % (key, v))
    for i, t in enumerate(ref["update_terms"]):
        need(_f32_exact(t), "update term %d exact in fp32" % i)
    need(_f32_exact(ref["grad"]) and _f32_exact(ref["w3p"]), "gradient and partial rows exact in fp32")
    need(_multiple(o["mom0"].double(), 1.0), "integer momentum")
    # softmax: m a power of two, the other logits at least 128 below
    m = ref["m"]
    need(bool(((m == 1) | (m == 2) | (m == 4) | (m == 8)).all()), "m in {1, 2, 4, 8}")
    need(float(ref["gap"].min()) >= LOGIT_GAP, "non-maximal logits at least 128 below")
    # not vacuous
    need(min(s["label_among"], s["label_not_among"], s["dz_zero"]) >= 0.25, "label among / not among the maxima, dZ = 0: 1/4 each")
    need(0.25 <= s["relu1_on"] <= 0.75 and 0.25 <= s["relu2_on"] <= 0.75, "ReLUs on for 1/4 .. 3/4")
    need(s["p1_zero"] >= 0.005, "0.5 % of layer-1 pre-activations exactly 0")
    need(int((ref["xu"].sum(0) == 0).sum()) == 0, "no zero column of X")
    need(int((ref["dh1"] == 0).all(0).sum()) == 0, "no zero column of dH1")
    need(int((ref["dh2"] == 0).all(0).sum()) == 0, "no zero column of dH2")
    need(s["dw1_nonzero"] >= 0.75 and s["dw2_nonzero"] >= 0.75, "3/4 of dW1 and dW2 nonzero")
    need(s["w2_rounds"] >= 0.25, "1/4 of the updated W2 not bf16 values")
    need(s["w1_rounds"] >= 0.25, "1/4 of the updated W1 not fp16 values")
    if case.x_step > 1:
        need(int(ref["xu"].max()) >= 128, "bytes with the high bit set")
    return s


def check_table_bounds(refs: dict) -> None:
    """Across the cases: each of m = 1, 2, 4 in at least 1/16 of some case's rows, m = 8 in the
    eight-way case."""
    for k in (1, 2, 4):
        assert max(r["shares"]["m%d" % k] for r in refs.values()) >= 1 / 16, k
    assert refs["T128"]["shares"]["m8"] >= 1 / 16, refs["T128"]["shares"]


# ---------------------------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------------------------
@dataclass
class Mismatch:
    what: str
    count: int
    total: int
    index: tuple
    got: float
    want: float
    note: str = ""

    def __str__(self):
        s = "%s: %d of %d elements differ; first at %s: got %r, want %r" % (
            self.what, self.count, self.total, self.index, self.got, self.want)
        return s + ("; " + self.note if self.note else "")


def _first(bad, shape):
    flat = int(torch.nonzero(bad.reshape(-1))[0])
    idx, rem = [], flat
    for dim in reversed(shape):
        idx.append(rem % dim)
        rem //= dim
    return flat, tuple(reversed(idx))


def compare(got, want, what: str = "", bm: int = 0, bound=None):
    """None when ``got`` equals the float64 ``want`` element for element (``torch.equal``, no
    tolerance; a NaN never equals), else a :class:`Mismatch` with the count and the first
    differing index.  bm: the tensor is [batch rows, columns] of the rows kernel with that tile
    height, and the note names the workgroup, the row inside it and the wave (64 columns).
    bound: a float64 tensor of per-element bounds instead of equality (the loss)."""
    g = got.detach().to("cpu", torch.float64).reshape(want.shape)
    if bound is None:
        if torch.equal(g, want):
            return None
        bad = (g != want) | torch.isnan(g)
    else:
        bad = ~((g - want).abs() <= bound)
        if not bool(bad.any()):
            return None
    flat, idx = _first(bad, want.shape)
    note = ""
    if bm and want.dim() == 2:
        note = "rows workgroup %d row %d (fragment row %d)" % (idx[0] // bm, idx[0] % bm, idx[0] % 16)
        if want.shape[1] == M.HIDDEN:
            note += ", wave %d column %d" % (idx[1] // 64, idx[1] % 64)
    if bound is not None:
        note = (note + "; " if note else "") + "bound %r" % float(bound.reshape(-1)[flat])
    return Mismatch(what, int(bad.sum()), want.numel(), idx, float(g.reshape(-1)[flat]), float(want.reshape(-1)[flat]), note)


def compare_flat(got, want, what: str = ""):
    """:func:`compare` of a flat parameter-shaped vector, tensor by tensor of ``param_layout()``:
    a list of mismatches whose index is (row, column) of the named tensor."""
    g = got.detach().to("cpu", torch.float64)
    out = []
    for name, shape, off, n in M.param_layout():
        m = compare(g[off:off + n], want[off:off + n].view(shape), "%s %s" % (what, name))
        if m is not None:
            out.append(m)
    return out


def frag_index(n_rows: int, n_cols: int, ks_per_row: int) -> torch.Tensor:
    """frag_off(n, k, ks_per_row) of mlp_fused.hip for n < n_rows, k < n_cols: where element
    [n][k] of a fragment-ordered shadow lies."""
    n = torch.arange(n_rows)[:, None]
    k = torch.arange(n_cols)[None, :]
    return ((n >> 4) * ks_per_row + (k >> 5)) * 512 + ((((k & 31) >> 3) << 4) | (n & 15)) * 8 + (k & 7)


def decode_frag(buf, n_rows: int, n_cols: int, ks_per_row: int):
    """The [n_rows][n_cols] matrix a fragment-ordered shadow holds (the inverse of frag_off), and
    the number of non-zero elements outside it (padding: must stay zero)."""
    flat = buf.detach().cpu().reshape(-1)
    idx = frag_index(n_rows, n_cols, ks_per_row)
    rest = flat.clone()
    rest[idx.reshape(-1)] = 0
    return flat[idx], int((rest != 0).sum())


# ---------------------------------------------------------------------------------------------
# drivers (GPU)
# ---------------------------------------------------------------------------------------------
def _trainer(case: Case, slices=None, **kw):
    class ExactTrainer(M.FusedMLPTrainer):
        """The trainer with the case's power-of-two scales as its launch arguments."""
        grad_scale = property(lambda self: case.grad_scale)
        dh1_scale = property(lambda self: case.dh1_scale)

    o = operands(case)
    tr = ExactTrainer(batch=case.batch, flat=o["flat"], lr=LR, momentum=MU, weight_decay=WD, slices=slices, **kw)
    tr.xa, tr.xb = case.xa, case.xb  # before the first launch that reads them
    tr._lkey = None
    tr.mom[:M.N_PARAMS].copy_(o["mom0"])
    tr.load_shard(o["x"], o["y"])
    tr.cursor.fill_(case.cursor)
    return tr


class _Setup:
    """The process-wide switches of a run: the rows tile and the X layout; restored on exit."""

    def __init__(self, case: Case, xt: bool):
        self.case, self.xt = case, xt

    def __enter__(self):
        from ..ops import _native

        self.old = os.environ.get("SL_MLP_XTILE")
        os.environ["SL_MLP_XTILE"] = "1" if self.xt else "0"
        _native.call("sl_mlp_set_rows_bm", self.case.force_bm)

    def __exit__(self, *exc):
        from ..ops import _native

        _native.call("sl_mlp_set_rows_bm", 0)
        if self.old is None:
            os.environ.pop("SL_MLP_XTILE", None)
        else:
            os.environ["SL_MLP_XTILE"] = self.old


def _check_launcher(case, tr, want_slices, xt, fails):
    from ..ops import _native

    bm = int(_native.lib().sl_mlp_rows_bm(case.batch))
    if bm != case.bm:
        fails.append("rows tile %d, the table says %d" % (bm, case.bm))
    if tr.slices != want_slices:
        fails.append("%d split-K slices, the table says %d" % (tr.slices, want_slices))
    if (tr.xt is not None) != xt:
        fails.append("tiled shard %s, asked for %s" % (tr.xt is not None, xt))
    return {"bm": bm, "slices": tr.slices, "xt": tr.xt is not None}


def run_case(case: Case, xt: bool = True) -> dict:
    """Rows (training and evaluation form), weight gradient and slab reduce of one case, for each
    slice count of the table, every buffer compared with the reference.  Returns {"failures":
    [str], "maxima": {...}, "shares": {...}, "ran": [{bm, slices, xt}], "loss_dev": worst
    |loss - reference| / bound}."""
    ref = reference(case)
    check_case_bounds(case, ref)
    o = operands(case)
    fails, ran, loss_dev = [], [], 0.0
    lo = (case.cursor % (case.rows // case.batch)) * case.batch
    xb, yb = o["x"][lo:lo + case.batch], o["y"][lo:lo + case.batch]

    def check(m):
        for one in (m if isinstance(m, list) else [m]):
            if one is not None:
                fails.append("[%s %s] %s" % (case.name, "xt" if xt else "rowmajor", one))

    def loss_check(got, what):
        nonlocal loss_dev
        dev = (got.detach().cpu().double() - ref["loss"]).abs() / ref["loss_bound"]
        loss_dev = max(loss_dev, float(dev.max()))
        check(compare(got, ref["loss"], what, bound=ref["loss_bound"]))

    nan = float("nan")
    with _Setup(case, xt):
        for req, want_slices in case.slices:
            tr = _trainer(case, slices=req)
            ran.append(_check_launcher(case, tr, want_slices, xt, fails))
            lc = tr._launches()
            for t in (tr.h1t, tr.dh2t, tr.dh1t, tr.loss, tr.correct, tr.grad):
                t.fill_(nan)  # every element must be written
            tr.w3p.zero_()  # one partial row per workgroup: fewer than the buffer holds at 128 rows
            lc["rows"]()
            torch.cuda.synchronize()
            check(compare(tr.h1t, ref["h1"], "h1t", bm=case.bm))
            check(compare(tr.dh2t, ref["dh2"], "dh2t", bm=case.bm))
            check(compare(tr.dh1t.view(torch.float16).double() / case.dh1_scale, ref["dh1"], "dh1t / dh1_scale", bm=case.bm))
            check(compare(tr.correct, ref["correct"], "correct"))
            loss_check(tr.loss, "loss")
            nrow = case.batch // case.bm
            w3p = tr.w3p.cpu().double()
            for name, a, b in (("dW3", 0, M.CLASSES * M.HIDDEN), ("db3", M.CLASSES * M.HIDDEN, W3P_N),
                               ("db1", W3P_DB1, W3P_DB2), ("db2", W3P_DB2, M.W3P_LD)):
                check(compare(w3p[:nrow, a:b], ref["w3p"][:, a:b], "w3p partial rows, %s" % name))
                check(compare(w3p[:, a:b].sum(0), ref["w3p"][:, a:b].sum(0), "w3p %s summed over rows" % name))
            lc["wgrad"]()
            lc["reduce"]()
            torch.cuda.synchronize()
            check(compare_flat(tr.grad[:M.N_PARAMS], ref["grad"], "grad (%d slices)" % tr.slices))
            if int(tr.cursor.item()) != case.cursor:
                fails.append("cursor moved to %d before the update" % int(tr.cursor.item()))
        # evaluation form: logits alone, then per-row loss / correct with the logits
        check(compare(tr.logits(xb), ref["z"], "logits (evaluation form)", bm=case.bm))
        rows = case.batch
        loss = torch.full((rows,), nan, device=tr.device)
        corr = torch.full((rows,), nan, device=tr.device)
        out = torch.full((rows, M.CLASSES), nan, device=tr.device)
        tr._eval_rows(tr._eval_set(False), xb.to(tr.device).contiguous(), yb.to(tr.device).contiguous(), rows,
                      loss, corr, logits=out)
        torch.cuda.synchronize()
        check(compare(out, ref["z"], "logits (evaluation form, with loss)", bm=case.bm))
        check(compare(corr, ref["correct"], "correct (evaluation form)"))
        loss_check(loss, "loss (evaluation form)")
    return {"name": case.name, "failures": fails, "maxima": ref["maxima"], "sumabs": ref["sumabs"],
            "shares": ref["shares"], "ran": ran, "loss_dev": loss_dev}


UPDATE_FORMS = ("sgd", "reduce+update", "opt")


def _update_state(tr) -> dict:
    """What an update leaves behind, decoded: parameters, momentum, the five shadows as matrices,
    the W1 row totals, and the padding that must have stayed zero."""
    st = {"params": tr.params[:M.N_PARAMS].cpu().double(), "mom": tr.mom[:M.N_PARAMS].cpu().double(),
          "pad": int((tr.params[M.N_PARAMS:] != 0).sum())}
    for key, t, shape in (("w1h", tr.w1h.view(torch.float16), (M.HIDDEN, M.D_IN, KS1)),
                          ("w2h", tr.w2h, (M.HIDDEN, M.HIDDEN, KS2)), ("w2th", tr.w2th, (M.HIDDEN, M.HIDDEN, KS2)),
                          ("w3h", tr.w3h, (M.CLASSES, M.HIDDEN, KS2)), ("w3th", tr.w3th, (M.HIDDEN, M.CLASSES, 1))):
        mat, rest = decode_frag(t, *shape)
        st[key] = mat.double()
        st["pad"] += rest
    st["r1"] = tr.r1p.cpu().view(M.HIDDEN, M.R1_BLK).sum(1)
    return st


def run_update(case: Case) -> dict:
    """One step each, on a fresh trainer from the preset integer momentum, through the fused "sgd"
    launch, "reduce" then "update", and sl_mlp_opt under the scheduled-SGD rule with a constant
    table; every piece of state against the reference and the three against each other; then the
    updated trainer's logits against a trainer freshly built from its parameters."""
    ref = reference(case)
    check_case_bounds(case, ref)
    o = operands(case)
    fails, states, ran = [], {}, []
    lo = (case.cursor % (case.rows // case.batch)) * case.batch
    xb = o["x"][lo:lo + case.batch]
    want = {"params": ref["params"], "mom": ref["mom"], "w1h": ref["w1h"], "w2h": ref["w2h"], "w2th": ref["w2h"].t(),
            "w3h": ref["w3h"], "w3th": ref["w3h"].t()}
    with _Setup(case, True):
        for form in UPDATE_FORMS:
            # (a one-step warm-up makes the rule "scheduled": the table is [lr, lr])
            tr = _trainer(case, **({"lr_warmup_steps": 1} if form == "opt" else {}))
            ran.append(_check_launcher(case, tr, case.slices[-1][1], True, fails))
            lc = tr._launches()
            if form == "opt":
                if lc["sgd"].name != "sl_mlp_opt" or tr.lr_tab is None or not bool((tr.lr_tab == LR).all()):
                    fails.append("opt: not the scheduled rule with a constant table")
            lc["rows"]()
            lc["wgrad"]()
            if form == "reduce+update":
                lc["reduce"]()
                lc["update"]()
            else:
                lc["sgd"]()
            torch.cuda.synchronize()
            st = states[form] = _update_state(tr)
            tag = "[%s update %s] " % (case.name, form)
            for key in ("params", "mom"):
                fails += [tag + str(m) for m in compare_flat(st[key], want[key], key)]
            for key in ("w1h", "w2h", "w2th", "w3h", "w3th"):
                m = compare(st[key], want[key], key + " (decoded)")
                if m is not None:
                    fails.append(tag + str(m))
            if not torch.equal(st["r1"], ref["r1"]):
                bad = (st["r1"] != ref["r1"]).nonzero().reshape(-1)
                fails.append(tag + "r1p row totals: %d of %d rows differ; first at row %d: got %d, want %d" % (
                    bad.numel(), M.HIDDEN, int(bad[0]), int(st["r1"][bad[0]]), int(ref["r1"][bad[0]])))
            if st["pad"]:
                fails.append(tag + "%d padding elements of the parameters / shadows are not zero" % st["pad"])
            if int(tr.cursor.item()) != case.cursor + 1:
                fails.append(tag + "cursor %d, want %d" % (int(tr.cursor.item()), case.cursor + 1))
            if form == "opt" and int(tr.opt_step.item()) != 1:
                fails.append(tag + "opt_step %d, want 1" % int(tr.opt_step.item()))
            # the shadows the update wrote serve the next forward as a fresh trainer's do
            fresh = M.FusedMLPTrainer(batch=case.batch, flat=tr.get_flat())
            fresh.xa, fresh.xb = case.xa, case.xb
            if not torch.equal(tr.logits(xb), fresh.logits(xb)):
                fails.append(tag + "logits after the update differ from a trainer built from get_flat()")
        for form in UPDATE_FORMS[1:]:
            for key, v in states[form].items():
                a = states[UPDATE_FORMS[0]][key]
                if not (torch.equal(a, v) if torch.is_tensor(v) else a == v):
                    fails.append("[%s] %s of the %s and the %s update differ" % (case.name, key, UPDATE_FORMS[0], form))
    return {"name": case.name, "failures": fails, "ran": ran, "shares": ref["shares"]}
