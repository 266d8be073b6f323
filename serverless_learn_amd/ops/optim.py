"""K5: the optimizer.  The update rules' semantics in one place (float64 reference functions
the CPU trainers run and the GPU tests compare against), the hyper-parameter bundle every
trainer shares, and the flat fused update kernels (one launch for a whole model's vector).

Two rules: momentum SGD (``torch.optim.SGD``, dampening 0, no nesterov) and AdamW
(``torch.optim.AdamW``: decoupled weight decay, bias correction, no amsgrad).  Both take their
learning rate from :func:`lr_at`: linear warm-up, then constant, linear or cosine decay.  On the
GPU the step number is a device-resident counter, so a captured graph replays with a moving
learning rate; the schedule reaches the kernels as an fp32 table of ``lr_at`` values.

Either rule may be preceded by global-norm gradient clipping (``clip_grad_norm``,
``torch.nn.utils.clip_grad_norm_``): :func:`clip_grad_` is its reference, and
:func:`clip_grad_norm_flat` the two-launch kernel that a captured graph replays.

Gradient accumulation (``accum_steps`` micro-batches per update) sums the micro-gradients ahead of
all that with :func:`accum_flat`, one fp32 add per element in a fixed order.

Weight decay may differ by parameter class (``norm_weight_decay``, ``bias_weight_decay``:
torchvision's ``set_weight_decay``): :func:`decay_class_map` gives every 64-element block of a
trainer's flat vector its class, :func:`decay_vector` the per-element decay the reference rules
take, and the ``*_groups`` launches read the same map on the device.

``optimizer="lars"`` (ResNet trainers) is momentum SGD whose decayed gradient is scaled per weight
tensor by a trust ratio of the tensor's and its gradient's norms: :func:`lars_update` is its
reference, :func:`lars_plan` cuts the flat vector into the chunks whose sums of squares
:func:`lars_norms` takes, :func:`lars_trust` folds them per tensor and :func:`sgd_flat_lars` is the
update launch (csrc/kernels/lars.hip).

``optimizer="muon"`` (ResNet trainers) keeps momentum SGD's state, but updates every conv weight
but the stem's, seen as the matrix ``[cout, k k cin]`` the flat vector stores, with its momentum
orthogonalised by Newton-Schulz iterations in bf16: :func:`newton_schulz` and :func:`muon_update`
are the reference, :func:`muon_plan` the host side (tensors, block map, tile tables) and
:func:`muon_prep`, :func:`muon_gram`, :func:`muon_poly`, :func:`muon_apply` and
:func:`sgd_flat_muon` the grouped launches (csrc/kernels/muon.hip).

Adaptive gradient clipping (``agc_clip``, under any rule; ResNet trainers) runs ahead of the global
clip: :func:`agc_clip_reference` is its float64 definition, :func:`agc_plan` its units (every conv
filter row, every norm vector) and :func:`agc_clip_flat` the one grouped launch
(csrc/kernels/agc.hip).

Sharpness-aware minimization (``sam_rho``, under any rule; ResNet trainers) takes the update's gradient
at weights perturbed along the first pass's local gradient: :func:`sam_perturb_reference` is the float64
definition of the perturbation, and :func:`sam_norms`, :func:`sam_scale` and :func:`sam_perturb` its
three launches (csrc/kernels/sam.hip); the way back is :func:`accum_flat` from the saved vector.

A weight EMA (``ema_decay``) follows every update: :func:`ema_update_` is its reference,
:func:`ema_table` the per-step coefficients and :func:`ema_flat` the one launch that applies them and
advances its own device-resident counter.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as N

OPTIMIZERS = ("sgd", "adamw", "lars", "muon")
SCHEDULES = ("constant", "linear", "cosine")

# update-kernel rules (csrc/kernels/mlp_fused.hip)
RULE_SGD, RULE_SGD_LR, RULE_ADAMW = 0, 1, 2


# ---- semantics ----
def lr_at(step: int, lr: float, schedule: str = "constant", warmup_steps: int = 0, decay_steps: int = 0,
          min_ratio: float = 0.0) -> float:
    """Learning rate of 0-based ``step`` (the number of updates already applied), in float64.

    ``step < warmup_steps``: ``lr (step + 1) / warmup_steps``.  After that, with
    ``p = min(1, (step - warmup_steps) / max(1, decay_steps - warmup_steps))`` and
    ``r = min_ratio``: ``constant`` 1, ``linear`` ``r + (1 - r)(1 - p)``, ``cosine``
    ``r + (1 - r) (1 + cos(pi p)) / 2``; past ``decay_steps`` it stays at ``r lr``."""
    if schedule not in SCHEDULES:
        raise ValueError(f"unknown lr_schedule {schedule!r} (choose from {SCHEDULES})")
    step, warmup_steps, decay_steps = int(step), int(warmup_steps), int(decay_steps)
    if schedule != "constant" and decay_steps <= 0:
        raise ValueError(f"lr_schedule {schedule!r} needs lr_decay_steps > 0 (or max_steps, which it defaults to)")
    if step < warmup_steps:
        return float(lr) * (step + 1) / warmup_steps
    if schedule == "constant":
        return float(lr)
    p = min(1.0, (step - warmup_steps) / max(1, decay_steps - warmup_steps))
    r = float(min_ratio)
    shape = 1.0 - p if schedule == "linear" else 0.5 * (1.0 + math.cos(math.pi * p))
    return float(lr) * (r + (1.0 - r) * shape)


def sgd_update(flat, mom, grad, lr, momentum, weight_decay):
    """torch.optim.SGD semantics (dampening 0, no nesterov), in place.  ``weight_decay``: a scalar
    or one value per element (:func:`decay_vector`), taken in ``flat``'s precision as a scalar is."""
    if torch.is_tensor(weight_decay):
        weight_decay = weight_decay.to(flat.dtype)
    d = grad + weight_decay * flat
    if mom is not None:
        mom.mul_(momentum).add_(d)
        d = mom
    flat.sub_(lr * d)


def adamw_update(flat, m, v, grad, lr_t, beta1, beta2, eps, weight_decay, t):
    """torch.optim.AdamW semantics (no amsgrad), in place; ``t`` = step + 1.  ``weight_decay``: a
    scalar or one float64 value per element (:func:`decay_vector`); either way ``1 - lr_t wd`` is
    formed in float64 and rounded once to ``flat``'s precision."""
    keep = 1.0 - lr_t * weight_decay
    flat.mul_(keep.to(flat.dtype) if torch.is_tensor(keep) else keep)
    m.mul_(beta1).add_(grad, alpha=1.0 - beta1)
    v.mul_(beta2).addcmul_(grad, grad, value=1.0 - beta2)
    denom = v.sqrt().div_(math.sqrt(1.0 - beta2 ** t)).add_(eps)
    flat.addcdiv_(m, denom, value=-lr_t / (1.0 - beta1 ** t))


# ---- per-class weight decay ----
# Every element of a flat parameter vector has one of three classes; a class is constant over a
# DECAY_BLOCK-element block, because every tensor of the vectors starts on such a boundary.
DECAY_CLASSES = ("weight", "norm", "bias")
CLS_WEIGHT, CLS_NORM, CLS_BIAS = 0, 1, 2
DECAY_BLOCK = 64


def check_group_decay(name: str, v) -> float | None:
    """``norm_weight_decay`` / ``bias_weight_decay``: None (follow ``weight_decay``) or a finite
    float >= 0."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError(f"{name} must be None (follow weight_decay) or a finite number >= 0, got {v!r}")
    return float(v)


def decay_class_map(layout, n: int, norm=()) -> np.ndarray:
    """The class of every :data:`DECAY_BLOCK`-element block of a flat vector of ``n`` elements, as
    uint8: ``layout`` is a trainer's ``layout()`` (``[name, shape, offset]`` per tensor) and
    ``norm`` the names of its normalisation layers' tensors (scale and shift: class 1).  Any other
    tensor named ``*.bias`` is class 2 and the rest class 0.  Alignment padding takes the class of
    the tensor it follows.  Every tensor must start on a block boundary."""
    norm = set(norm)
    cls = np.zeros((int(n) + DECAY_BLOCK - 1) // DECAY_BLOCK, dtype=np.uint8)
    entries = sorted(layout, key=lambda e: e[2])
    assert entries and entries[0][2] == 0, "the first tensor starts the vector"
    for i, (name, shape, off) in enumerate(entries):
        assert off % DECAY_BLOCK == 0, f"{name} starts at {off}: not on a {DECAY_BLOCK}-element boundary"
        end = entries[i + 1][2] if i + 1 < len(entries) else int(n)
        assert off + math.prod(shape) <= end, f"{name} overlaps the tensor after it"
        c = CLS_NORM if name in norm else CLS_BIAS if name.endswith(".bias") else CLS_WEIGHT
        cls[off // DECAY_BLOCK:(end + DECAY_BLOCK - 1) // DECAY_BLOCK] = c
    assert not norm - {e[0] for e in entries}, "a normalisation tensor that is not in the layout"
    return cls


def trainer_class_map(trainer) -> np.ndarray:
    """:func:`decay_class_map` of a trainer: its ``layout()``, its ``norm_tensors()`` (the ResNets'
    BatchNorm scales and shifts; the MLP has none) and the length of its ``params``."""
    return decay_class_map(trainer.layout(), int(trainer.params.numel()), trainer.norm_tensors())


def decay_class_counts(cls: np.ndarray, n: int) -> tuple:
    """Elements of the first ``n`` in each class (padding counted with its tensor)."""
    per = np.repeat(np.asarray(cls), DECAY_BLOCK)[:int(n)]
    return tuple(int((per == c).sum()) for c in range(len(DECAY_CLASSES)))


def decay_vector(cls, n: int, decays, device="cpu") -> torch.Tensor:
    """The float64 weight decay of each of ``n`` elements: ``decays[class]``."""
    per = torch.as_tensor(np.asarray(cls)).long().repeat_interleave(DECAY_BLOCK)[:int(n)]
    assert per.numel() == int(n), "the class map is shorter than the vector"
    return torch.tensor([float(d) for d in decays], dtype=torch.float64)[per].to(device)


# ---- LARS: layer-wise trust ratios (You et al. 2017; apex LARC's scaling without its clip) ----
LARS_CHUNK = 4096     # elements per chunk of the norms launch (csrc/kernels/lars.hip LARS_CHUNK)
LARS_NO_TENSOR = 0xFFFF  # block-map entry of a block no adapted tensor owns


def check_lars(eta, eps) -> None:
    """``lars_eta``: a finite float > 0; ``lars_eps``: a finite float >= 0."""
    num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)  # noqa: E731
    if not num(eta) or eta <= 0:
        raise ValueError(f"lars_eta must be a finite number > 0, got {eta!r}")
    if not num(eps) or eps < 0:
        raise ValueError(f"lars_eps must be a finite number >= 0, got {eps!r}")


@dataclass(frozen=True)
class LarsPlan:
    """:func:`lars_plan`'s result.  ``names``: the T adapted tensors (class 0: conv and linear
    weights) in offset order; ``tensors``: int32 ``[T][4]`` = (offset, numel, first chunk, chunk
    count); ``chunks``: int32 ``[C][2]`` = (offset, count); ``block_map``: uint16 per 64-element
    block, the adapted tensor that owns it or :data:`LARS_NO_TENSOR`; ``cls``: the
    :func:`decay_class_map` of the same layout; ``n``: the vector's length."""
    names: tuple
    tensors: np.ndarray
    chunks: np.ndarray
    block_map: np.ndarray
    cls: np.ndarray
    n: int


def lars_plan(layout, n: int, norm=()) -> LarsPlan:
    """How the LARS launches see a flat vector of ``n`` elements (``layout``, ``norm``: as for
    :func:`decay_class_map`, which is asserted).  Every class-0 tensor is adapted: its real
    elements ``[off, off + numel)`` are cut into consecutive chunks of at most :data:`LARS_CHUNK`
    elements, none straddling a tensor, each starting on a 16-byte boundary (tensors start on
    64-element boundaries), only a tensor's last with a count that is no multiple of 4.  Padding
    belongs to the tensor it follows in the block map, and is in no chunk."""
    n = int(n)
    assert 0 < n < 2 ** 31, "the chunk table holds int32 offsets"
    cls = decay_class_map(layout, n, norm)
    entries = sorted(layout, key=lambda e: e[2])
    names, tensors, chunks = [], [], []
    block_map = np.full(cls.shape, LARS_NO_TENSOR, dtype=np.uint16)
    for i, (name, shape, off) in enumerate(entries):
        numel = math.prod(shape)
        if cls[off // DECAY_BLOCK] != CLS_WEIGHT or numel == 0:
            continue
        end = entries[i + 1][2] if i + 1 < len(entries) else n
        block_map[off // DECAY_BLOCK:(end + DECAY_BLOCK - 1) // DECAY_BLOCK] = len(names)
        first = len(chunks)
        chunks += [(o, min(LARS_CHUNK, off + numel - o)) for o in range(off, off + numel, LARS_CHUNK)]
        tensors.append((off, numel, first, len(chunks) - first))
        names.append(name)
    assert 0 < len(names) < LARS_NO_TENSOR, "the block map names a tensor in 16 bits"
    return LarsPlan(tuple(names), np.array(tensors, dtype=np.int32).reshape(-1, 4),
                    np.array(chunks, dtype=np.int32).reshape(-1, 2), block_map, cls, n)


def lars_update(flat, mom, grad, lr_t, momentum, decay, tensors: LarsPlan, eta, eps, trust=None) -> list:
    """The LARS reference, in place, in float64 on the fp32 state (each stored value rounded once).
    For every adapted tensor ``T`` of the plan ``tensors``, over its real elements: ``wn = ||w||``,
    ``gn = ||g||``, ``trust_T = eta wn / (gn + wd wn + eps)`` where both norms are positive and 1
    otherwise, with ``wd = decay[0]``; every other element has trust 1.  Then element-wise, with
    ``c`` the element's class: ``d = trust_T (g + decay[c] w)``, ``mom = momentum mom + d``,
    ``w -= lr_t mom`` (``mom`` None: ``w -= lr_t d``).  Returns ``(wn, gn, trust)`` per adapted
    tensor, in the plan's order.  ``trust``: ratios to apply in place of the computed ones (a GPU
    test passes the kernel's own fp32 values, so that its element-wise bound holds no norm error)."""
    plan = tensors
    n = plan.n
    w, g = flat[:n].double(), grad[:n].double()
    rows = []
    for t, (off, numel, _, _) in enumerate(plan.tensors.tolist()):
        wn = float(torch.linalg.vector_norm(w[off:off + numel]))
        gn = float(torch.linalg.vector_norm(g[off:off + numel]))
        tr = eta * wn / (gn + float(decay[0]) * wn + eps) if wn > 0 and gn > 0 else 1.0
        rows.append((wn, gn, tr if trust is None else float(trust[t])))
    scale = torch.tensor([r[2] for r in rows] + [1.0], dtype=torch.float64)
    owner = torch.as_tensor(plan.block_map.astype(np.int64)).clamp_(max=len(rows))
    d = scale[owner.repeat_interleave(DECAY_BLOCK)[:n]] * (g + decay_vector(plan.cls, n, decay) * w)
    if mom is not None:
        d = momentum * mom[:n].double() + d
        mom[:n] = d.to(mom.dtype)
    flat[:n] = (w - lr_t * d).to(flat.dtype)
    return rows


# ---- Muon: momentum orthogonalised by Newton-Schulz (Jordan et al. 2024) ----
NS_COEFFS = (3.4445, -4.7750, 2.0315)  # (a, b, c) of X <- a X + (b A + c A A) X, A = X X^T
MUON_EPS = 1e-7       # added to ||u||_F
MUON_TILE = 64        # both sides of a Muon tensor are multiples of it (csrc/kernels/muon.hip MU_TILE)
MUON_CHUNK = MUON_TILE * MUON_TILE  # elements per chunk of the momentum launch (sl_muon_chunk)
MUON_MAX_SIDE = 512   # the working (wide-orientation) row count's limit
MUON_KSLICE = 512     # columns per split-K slice of the Gram launch
MUON_EXCLUDE = ("stem.weight", "fc.weight")  # multi-dimensional weights that stay on the SGD rule


def check_muon(lr_ratio, nesterov, ns_steps) -> None:
    """``muon_lr_ratio``: a finite float > 0; ``muon_nesterov``: a bool; ``muon_ns_steps``: an
    integer in 1..8."""
    r = lr_ratio
    if isinstance(r, bool) or not isinstance(r, (int, float)) or not math.isfinite(r) or r <= 0:
        raise ValueError(f"muon_lr_ratio must be a finite number > 0, got {r!r}")
    if not isinstance(nesterov, (bool, np.bool_)):
        raise ValueError(f"muon_nesterov must be a bool, got {nesterov!r}")
    k = ns_steps
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 8:
        raise ValueError(f"muon_ns_steps must be an integer in 1..8, got {k!r}")


def _bf16(x: torch.Tensor) -> torch.Tensor:
    return x.float().bfloat16().double()


def newton_schulz(u: torch.Tensor, steps: int = 5, emulate: bool = False) -> torch.Tensor:
    """``steps`` Newton-Schulz iterations on the matrix ``u``, in float64: ``X = u / (||u||_F +
    1e-7)``, transposed if it is tall, then ``A = X X^T``, ``B = b A + c A A``, ``X = a X + B X``
    with :data:`NS_COEFFS`, transposed back.  ``emulate``: round to bf16 at the four stores the
    kernels make (X0, A, B and every X); without it nothing is rounded."""
    a, b, c = NS_COEFFS
    rnd = _bf16 if emulate else (lambda x: x)
    u = u.double()
    X = rnd(u / (torch.linalg.vector_norm(u) + MUON_EPS))
    tall = X.shape[0] > X.shape[1]
    if tall:
        X = X.T
    for _ in range(int(steps)):
        A = rnd(X @ X.T)
        B = rnd(b * A + c * (A @ A))
        X = rnd(a * X + B @ X)
    return (X.T if tall else X).contiguous()


def fma32(a: float, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """fp32 ``fma(a, x, y)`` of fp32 tensors, exactly: the product is exact in float64, the sum is
    rounded to odd there (its TwoSum error says which way), and float64 -> fp32 rounds once."""
    p, y = float(np.float32(a)) * x.double(), y.double()
    s = p + y
    bb = s - p
    err = (p - (s - bb)) + (y - bb)
    odd = (err != 0) & ((s.view(torch.int64) & 1) == 0)
    toward = torch.where(err > 0, math.inf, -math.inf).to(torch.float64)
    return torch.where(odd, torch.nextafter(s, toward), s).float()


@dataclass(frozen=True)
class MuonPlan:
    """:func:`muon_plan`'s result.  ``names``: the T Muon tensors in offset order; ``tensors``:
    int32 ``[T][12]`` = (offset, m, n, transposed, x offset, a offset, partials offset, slices,
    first chunk, chunk count, columns per slice, 0), where the work buffers hold tensor ``t`` in
    the wide orientation (``min(m, n)`` rows) at ``x offset``, its Gram matrices at ``a offset``
    and its split-K partials at ``partials offset``; ``chunks``: int32 ``[C]`` offsets of
    :data:`MUON_CHUNK` elements; ``block_map``: as :class:`LarsPlan`'s; ``cls``: the
    :func:`decay_class_map`; the int32 ``[.][4]`` tile tables ``tiles`` (tensor, i, j, 0: every
    64 x 64 tile of every X), ``gram_tiles`` (tensor, i, j <= i, slice), ``tri_tiles`` (tensor, i,
    j <= i, 0) and ``poly_tiles`` (tensor, i, j, 0); ``x_elems``, ``a_elems``, ``ws_floats``: the
    work buffers' sizes; ``n``: the vector's length."""
    names: tuple
    tensors: np.ndarray
    chunks: np.ndarray
    block_map: np.ndarray
    cls: np.ndarray
    tiles: np.ndarray
    gram_tiles: np.ndarray
    tri_tiles: np.ndarray
    poly_tiles: np.ndarray
    x_elems: int
    a_elems: int
    ws_floats: int
    n: int


def muon_plan(layout, n: int, norm=(), exclude=MUON_EXCLUDE) -> MuonPlan:
    """How the Muon launches see a flat vector of ``n`` elements (``layout``, ``norm``: as for
    :func:`decay_class_map`).  Every class-0 tensor of two or more dimensions that ``exclude`` does
    not name is a Muon tensor, the matrix ``[shape[0], prod(shape[1:])]``; both sides must be
    multiples of :data:`MUON_TILE` and the smaller at most :data:`MUON_MAX_SIDE` (ValueError)."""
    n = int(n)
    assert 0 < n < 2 ** 31, "the tables hold int32 offsets"
    cls = decay_class_map(layout, n, norm)
    names, tensors, chunks = [], [], []
    tiles, gram, tri, poly = [], [], [], []
    block_map = np.full(cls.shape, LARS_NO_TENSOR, dtype=np.uint16)
    xoff = aoff = poff = 0
    for name, shape, off in sorted(layout, key=lambda e: e[2]):
        if len(shape) < 2 or name in exclude or cls[off // DECAY_BLOCK] != CLS_WEIGHT:
            continue
        m, k = int(shape[0]), math.prod(shape[1:])
        rows, cols = min(m, k), max(m, k)
        if m % MUON_TILE or k % MUON_TILE or not 0 < rows <= MUON_MAX_SIDE:
            raise ValueError(f"muon: {name} is {m} x {k}: both sides must be multiples of {MUON_TILE} and the "
                             f"smaller at most {MUON_MAX_SIDE}")
        t, kslice = len(names), min(MUON_KSLICE, cols)
        slices, rt, ct = -(-cols // kslice), rows // MUON_TILE, cols // MUON_TILE
        block_map[off // DECAY_BLOCK:(off + m * k) // DECAY_BLOCK] = t
        tensors.append((off, m, k, int(m > k), xoff, aoff, poff, slices, len(chunks), m * k // MUON_CHUNK, kslice, 0))
        chunks += range(off, off + m * k, MUON_CHUNK)
        tiles += [(t, i, j, 0) for i in range(rt) for j in range(ct)]
        tri += [(t, i, j, 0) for i in range(rt) for j in range(i + 1)]
        gram += [(t, i, j, s) for s in range(slices) for i in range(rt) for j in range(i + 1)]
        poly += [(t, i, j, 0) for i in range(rt) for j in range(rt)]
        names.append(name)
        xoff, aoff, poff = xoff + m * k, aoff + rows * rows, poff + slices * rows * rows
    assert 0 < len(names) < LARS_NO_TENSOR, "the block map names a tensor in 16 bits"
    assert max(xoff, poff) < 2 ** 31, "the tables hold int32 offsets"
    tab = lambda rows, w: np.array(rows, dtype=np.int32).reshape(-1, w)  # noqa: E731
    return MuonPlan(tuple(names), tab(tensors, 12), np.array(chunks, dtype=np.int32), block_map, cls, tab(tiles, 4),
                    tab(gram, 4), tab(tri, 4), tab(poly, 4), xoff, aoff, poff, n)


def muon_update(flat, mom, grad, lr_t, momentum, decay, plan: MuonPlan, lr_ratio=1.0, nesterov=True, ns_steps=5,
                only=None) -> list:
    """The Muon reference, in place.  For every tensor ``T`` of the plan (``only``: just those
    names; the others' weights are left alone, their momentum still moves), as ``W[m][n]``:
    ``mom = fma(mu, mom, g)`` in fp32 with ``mu = float32(momentum)``, ``u = fma(mu, mom, g)``
    (``nesterov``) or ``mom``, ``O = newton_schulz(u, ns_steps, emulate=True)`` and, in float64
    rounded once, ``w = w (1 - lr_t r decay[0]) - lr_t r sqrt(max(1, m / n)) O``.  Every other
    element takes :func:`lars_update`'s rule at trust 1 (``d = g + decay[c] w``, ``mom = momentum
    mom + d``, ``w -= lr_t mom``).  ``mom`` is required.  Returns ``||u||_F`` per Muon tensor."""
    n = plan.n
    w, g = flat[:n].double(), grad[:n].double()
    d = momentum * mom[:n].double() + g + decay_vector(plan.cls, n, decay) * w
    new_m, new_w = d.to(mom.dtype), (w - lr_t * d).to(flat.dtype)
    norms = []
    for name, (off, m, k, *_) in zip(plan.names, plan.tensors.tolist()):
        sl = slice(off, off + m * k)
        new_m[sl] = fma32(momentum, mom[sl], grad[sl])
        u = fma32(momentum, new_m[sl], grad[sl]) if nesterov else new_m[sl]
        norms.append(float(torch.linalg.vector_norm(u.double())))
        new_w[sl] = flat[sl]
        if only is None or name in only:
            o = newton_schulz(u.view(m, k), ns_steps, emulate=True).reshape(-1)
            step = lr_t * lr_ratio
            new_w[sl] = (w[sl] * (1.0 - step * float(decay[0])) - step * math.sqrt(max(1.0, m / k)) * o).to(flat.dtype)
    mom[:n], flat[:n] = new_m, new_w
    return norms


CLIP_EPS = 1e-6  # torch.nn.utils.clip_grad_norm_'s constant


def clip_grad_(g: torch.Tensor, max_norm: float) -> float:
    """``torch.nn.utils.clip_grad_norm_`` over one flat gradient, in place: with ``total`` the
    L2 norm of ``g`` (taken in float64), ``g *= min(1, max_norm / (total + 1e-6))``.  Returns
    ``total``, the norm before clipping; ``max_norm = inf`` measures and never scales."""
    total = float(torch.linalg.vector_norm(g.detach().double()))
    coef = min(1.0, float(max_norm) / (total + CLIP_EPS))
    g.mul_(coef)
    return total


# ---- adaptive gradient clipping (Brock et al. 2021; timm's adaptive_clip_grad) ----
AGC_FIELDS = 4         # ints per unit of the table (csrc/kernels/agc.hip AgcUnit)
AGC_UNITS_PER_WG = 4   # units per workgroup, one per wave (AGC_WAVES)
AGC_EXCLUDE = ("fc.weight", "fc.bias")  # the final linear layer is not clipped (the paper leaves it out)


def check_agc(clip, eps) -> None:
    """``agc_clip``: a finite float >= 0 (0: off); ``agc_eps``: a finite float > 0."""
    num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)  # noqa: E731
    if not num(clip) or clip < 0:
        raise ValueError(f"agc_clip must be a finite number >= 0 (0: off), got {clip!r}")
    if not num(eps) or eps <= 0:
        raise ValueError(f"agc_eps must be a finite number > 0, got {eps!r}")


@dataclass(frozen=True)
class AgcPlan:
    """:func:`agc_plan`'s result.  ``names``: the tensors that have units, in offset order; ``units``:
    int32 ``[U][4]`` = (offset, n, cin, cin_real), the longest first (a 1-D unit has ``cin = cin_real
    = n``); ``owner``: per unit, its tensor's index in ``names``; ``work``: int32 ``[W][2]`` = (first
    unit, unit count), one workgroup of the launch each; ``n``: the vector's length.  Everything that
    is reported per unit (the stats rows) is in ``units``' order."""
    names: tuple
    units: np.ndarray
    owner: np.ndarray
    work: np.ndarray
    n: int


def agc_plan(layout, n: int, convs, norm=()) -> AgcPlan:
    """The units of adaptive gradient clipping in a flat vector of ``n`` elements.  ``convs``: the conv
    banks (``ConvSpec``s: name, off, cout, k, cin, cin_real), every row ``W[co][k k cin]`` of which is
    one unit; ``norm``: the names, in ``layout`` (``[name, shape, offset]`` per tensor), of the
    normalisation layers' scales and shifts, each one unit as a whole.  Nothing else is clipped
    (:data:`AGC_EXCLUDE`).  The units are sorted longest first (stable: offset order within a
    length), so the launch's last workgroups hold the short ones.  Shapes are not judged here: the
    launcher refuses what the kernel does not serve."""
    n = int(n)
    assert 0 < n < 2 ** 31, "the unit table holds int32 offsets"
    at = {name: (shape, off) for name, shape, off in layout}
    tensors = [(c.off, c.name + ".weight", c.cout, c.k * c.k * c.cin, c.cin, c.cin_real) for c in convs]
    for name in norm:
        shape, off = at[name]
        tensors.append((off, name, 1, math.prod(shape), math.prod(shape), math.prod(shape)))
    tensors.sort()
    assert not {t[1] for t in tensors} & set(AGC_EXCLUDE), "the final linear layer is not clipped"
    names, units, owner = [], [], []
    for off, name, rows, k, cin, cin_real in tensors:
        assert name in at and at[name][1] == off and math.prod(at[name][0]) == rows * k, f"{name} is not the layout's"
        units += [(off + r * k, k, cin, cin_real) for r in range(rows)]
        owner += [len(names)] * rows
        names.append(name)
    assert units, "nothing to clip"
    order = sorted(range(len(units)), key=lambda i: -units[i][1])
    work = [(u, min(AGC_UNITS_PER_WG, len(units) - u)) for u in range(0, len(units), AGC_UNITS_PER_WG)]
    return AgcPlan(tuple(names), np.array([units[i] for i in order], dtype=np.int32).reshape(-1, AGC_FIELDS),
                   np.array([owner[i] for i in order], dtype=np.int32), np.array(work, dtype=np.int32).reshape(-1, 2), n)


def _agc_norms(x: torch.Tensor) -> torch.Tensor:
    """The L2 norm of every row of the float64 matrix ``x``, safe at both ends of the fp32 range:
    ``amax sqrt(sum (x / amax)^2)`` with ``amax = max |x|`` of the row.  A row of zeros has norm 0
    (no division); a row holding an Inf or a NaN has a NaN norm (``x * 0`` stands in for the
    quotient there), never ``+Inf``."""
    amax = x.abs().amax(dim=1)  # (a NaN propagates)
    ok = (amax > 0) & (amax < math.inf)
    q = torch.where(ok[:, None], x / torch.where(ok, amax, 1.0)[:, None], x * 0.0)
    return amax * (q * q).sum(dim=1).sqrt()


def agc_clip_reference(flat, grad, plan: AgcPlan, clip: float, eps: float = 1e-3) -> torch.Tensor:
    """Adaptive gradient clipping's definition, in place on the fp32 gradient ``grad``.  For every
    unit of ``plan``, over its real columns (``col % cin < cin_real``) and in float64: ``wn = ||w||``
    of ``flat``, ``gn = ||g||`` (:func:`_agc_norms`), ``t = clip max(wn, eps)`` (a NaN ``wn`` stays a
    NaN).  A unit is clipped iff ``gn > t`` -- so not at ``gn = 0`` and not with a NaN norm -- and
    then every stored element of it, padding columns included, becomes ``g * s`` in fp32 with ``s =
    float32(t / gn)``; a unit that is not clipped is not written.  Returns the float64 ``[U][3]``
    rows ``(wn, gn, s)`` in the plan's order, ``s = 1`` where nothing was clipped."""
    assert grad.dtype == torch.float32 and flat.numel() >= plan.n and grad.numel() >= plan.n
    units = torch.from_numpy(plan.units.astype(np.int64))
    rows = torch.ones(len(units), 3, dtype=torch.float64)
    for key in sorted({tuple(u[1:]) for u in plan.units.tolist()}):  # one gather per shape of unit
        k, cin, cin_real = key
        sel = ((units[:, 1:] == torch.tensor(key)).all(dim=1)).nonzero().reshape(-1)
        idx = (units[sel, 0][:, None] + torch.arange(k)[None, :]).to(grad.device)
        real = (torch.arange(k) % cin < cin_real).to(grad.device)
        g = grad[idx]
        wn, gn = _agc_norms(flat[idx][:, real].double()).cpu(), _agc_norms(g[:, real].double()).cpu()
        t = float(clip) * torch.where(wn < float(eps), float(eps), wn)
        clipped = gn > t
        s = torch.where(clipped, t / gn, 1.0).float()
        if bool(clipped.any()):
            c = clipped.to(grad.device)
            grad[idx[c]] = g[c] * s.to(grad.device)[c][:, None]
        rows[sel] = torch.stack([wn, gn, s.double()], dim=1)
    return rows


def agc_summary(plan: AgcPlan, rows) -> dict:
    """``{tensor name: (units, clipped units, smallest s)}`` from the ``(wn, gn, s)`` rows of one
    step (``s < 1`` marks a clipped unit)."""
    s = np.asarray(rows, dtype=np.float64).reshape(-1, 3)[:, 2]
    out = {}
    for t, name in enumerate(plan.names):
        mine = s[plan.owner == t]
        out[name] = (int(mine.size), int((mine < 1.0).sum()), float(mine.min()))
    return out


# ---- sharpness-aware minimization (Foret et al. 2021; ASAM: Kwon et al. 2021) ----
SAM_CHUNK = 4096   # elements per chunk of the norms launch (csrc/kernels/sam.hip SAM_CHUNK)
SAM_EPS = 1e-12    # added to the norm under rho


def check_sam(rho, adaptive, eta) -> None:
    """``sam_rho``: a finite float >= 0 (0: off); ``sam_adaptive``: a bool; ``sam_eta``: a finite
    float > 0."""
    num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)  # noqa: E731
    if not num(rho) or rho < 0:
        raise ValueError(f"sam_rho must be a finite number >= 0 (0: off), got {rho!r}")
    if not isinstance(adaptive, (bool, np.bool_)):
        raise ValueError(f"sam_adaptive must be a bool, got {adaptive!r}")
    if not num(eta) or eta <= 0:
        raise ValueError(f"sam_eta must be a finite number > 0, got {eta!r}")


def sam_perturb_reference(w: torch.Tensor, g: torch.Tensor, cls, rho: float, adaptive: bool = False,
                          eta: float = 0.01) -> tuple:
    """Sharpness-aware minimization's perturbed weights, in float64: ``(w', nrm, scale)``.  ``w``:
    the flat fp32 parameters; ``g``: the first pass's local ``dL/dw`` (0 in alignment padding); ``cls``:
    the :func:`decay_class_map` of the vector.  ``T_i = |w_i| + eta`` for a class-0 element of an
    ``adaptive`` step (ASAM, biases and norm parameters left non-adaptive) and 1 otherwise; ``nrm =
    sqrt(sum_i (T_i g_i)^2)``, summed per chunk of :data:`SAM_CHUNK` elements and the chunk sums then
    folded in chunk order; ``scale = rho / (nrm + 1e-12)``, or 0 where ``nrm`` is not finite (``w'`` is
    then ``w``: a non-finite gradient stays the clip's business); ``w'_i = float32(w_i + scale T_i T_i
    g_i)``, evaluated left to right and rounded once."""
    n = int(w.numel())
    w64, g64 = w.detach().double().reshape(-1), g.detach().double().reshape(-1)
    T = torch.ones_like(w64)
    if adaptive:
        per = torch.as_tensor(np.asarray(cls)).long().repeat_interleave(DECAY_BLOCK)[:n].to(w64.device)
        assert per.numel() == n, "the class map is shorter than the vector"
        T = torch.where(per == CLS_WEIGHT, w64.abs() + float(eta), T)
    t = T * g64
    sq = torch.cat([t * t, t.new_zeros(-n % SAM_CHUNK)]).view(-1, SAM_CHUNK)
    total = 0.0
    for p in sq.sum(dim=1).tolist():
        total += p
    nrm = math.sqrt(total)
    scale = float(rho) / (nrm + SAM_EPS) if math.isfinite(nrm) else 0.0
    if scale == 0.0:
        return w.detach().clone().reshape(-1), nrm, scale
    return (w64 + scale * T * T * g64).to(w.dtype), nrm, scale


EMA_WARMUP_OFFSET = 10   # warm-up: decay_t = min(decay, (1 + t) / (10 + t))
EMA_TABLE_MAX = 1 << 20  # entries of the warm-up table


def _ema_last(decay: float, warmup: bool) -> int:
    """T: the first update ``t`` at which the warm-up ``(1 + t) / (10 + t)`` has reached ``decay``
    (0 with warm-up off), ``max(0, ceil((10 D - 1) / (1 - D)))``; refuses a bad decay and a table
    past :data:`EMA_TABLE_MAX`."""
    d = float(decay)
    if not 0.0 <= d < 1.0:  # negative, NaN, or no averaging at all
        raise ValueError(f"ema_decay must be in [0, 1) (0: off), got {decay!r}")
    if not warmup or d == 0.0:
        return 0
    if (EMA_WARMUP_OFFSET * d - 1.0) / (1.0 - d) > EMA_TABLE_MAX:
        raise ValueError(f"ema_decay {decay!r}: its warm-up table would be longer than {EMA_TABLE_MAX} entries "
                         "(turn ema_warmup off)")
    reached = lambda t: (1 + t) / (EMA_WARMUP_OFFSET + t) >= d  # noqa: E731
    last = max(0, math.ceil((EMA_WARMUP_OFFSET * d - 1.0) / (1.0 - d)))
    while last > 0 and reached(last - 1):  # (the closed form, in floating point, may be one off)
        last -= 1
    while not reached(last):
        last += 1
    if last + 1 > EMA_TABLE_MAX:
        raise ValueError(f"ema_decay {decay!r}: its warm-up table would be longer than {EMA_TABLE_MAX} entries "
                         "(turn ema_warmup off)")
    return last


def ema_table_len(decay: float, warmup: bool = True) -> int:
    """Entries of :func:`ema_table` (0 with the EMA off); refuses what it refuses."""
    last = _ema_last(decay, warmup)
    return 0 if float(decay) == 0.0 else last + 1


def ema_table(decay: float, warmup: bool = True) -> np.ndarray:
    """``float32(1 - d_t)`` for EMA updates ``t = 0 .. T`` (each computed in float64 and rounded
    once), where ``d_t = min(decay, (1 + t) / (10 + t))`` with warm-up and ``decay`` without, and
    ``T`` is the first ``t`` at which the warm-up has reached ``decay``: every later update has the
    last entry's value, so the table is indexed with ``min(t, T)`` as ``lr_tab`` is.  Without
    warm-up it has one entry."""
    last = _ema_last(decay, warmup)
    if float(decay) == 0.0:
        raise ValueError("ema_decay 0 is off: there is no table")
    t = np.arange(last + 1, dtype=np.float64)
    d_t = np.minimum(float(decay), (1.0 + t) / (EMA_WARMUP_OFFSET + t)) if warmup else np.full(1, float(decay))
    return (1.0 - d_t).astype(np.float32)


def ema_update_(ema: torch.Tensor, w: torch.Tensor, omd) -> None:
    """The weight EMA's reference, in place: ``e <- e + omd * (w - e)`` as three fp32 operations,
    each rounded once (subtract, multiply, add; no fma), with ``omd = float32(1 - decay_t)``.
    ``w == e`` leaves ``e`` unchanged."""
    assert ema.dtype == torch.float32 and w.dtype == torch.float32 and ema.shape == w.shape
    d = torch.sub(w, ema)
    d.mul_(torch.as_tensor(omd, dtype=torch.float32, device=d.device))
    ema.add_(d)


@dataclass(frozen=True)
class OptSpec:
    """The optimizer hyper-parameters a trainer is built with (its keyword arguments)."""
    lr: float = 0.05
    momentum: float = 0.9
    weight_decay: float = 0.0
    optimizer: str = "sgd"
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1e-8
    lr_schedule: str = "constant"
    lr_warmup_steps: int = 0
    lr_decay_steps: int = 0
    lr_min_ratio: float = 0.0
    clip_grad_norm: float = 0.0  # max global L2 norm of the gradient (0: off; inf: measure only)
    ema_decay: float = 0.0       # weight EMA after every update (0: off); no rule or kernel choice depends on it
    ema_warmup: bool = True      # decay_t = min(ema_decay, (1 + t) / (10 + t))
    # the decay of BatchNorm scales and shifts / of the other biases (None: weight_decay); setting
    # either switches the decay groups on, even to weight_decay's own value
    norm_weight_decay: float | None = None
    bias_weight_decay: float | None = None
    # optimizer="lars": the trust coefficient, and a constant added to the trust ratio's denominator
    lars_eta: float = 0.001
    lars_eps: float = 0.0
    # optimizer="muon": the Muon tensors' lr over the schedule's, Nesterov momentum, Newton-Schulz iterations
    muon_lr_ratio: float = 1.0
    muon_nesterov: bool = True
    muon_ns_steps: int = 5
    # adaptive gradient clipping ahead of clip_grad_norm and the update, under any rule (ResNet trainers): every
    # conv filter and norm vector of the gradient is held to agc_clip * max(its weights' norm, agc_eps) (0: off)
    agc_clip: float = 0.0
    agc_eps: float = 1e-3
    # sharpness-aware minimization, under any rule (ResNet trainers): the update's gradient is taken at weights moved
    # sam_rho along the first pass's local gradient (0: off); sam_adaptive: ASAM, the conv / linear weights' move
    # scaled element-wise by |w| + sam_eta.  No rule or kernel choice depends on these
    sam_rho: float = 0.0
    sam_adaptive: bool = False
    sam_eta: float = 0.01

    def __post_init__(self):
        check_group_decay("norm_weight_decay", self.norm_weight_decay)
        check_group_decay("bias_weight_decay", self.bias_weight_decay)
        if self.optimizer not in OPTIMIZERS:
            raise ValueError(f"unknown optimizer {self.optimizer!r} (choose from {OPTIMIZERS})")
        check_lars(self.lars_eta, self.lars_eps)
        check_muon(self.muon_lr_ratio, self.muon_nesterov, self.muon_ns_steps)
        check_agc(self.agc_clip, self.agc_eps)
        check_sam(self.sam_rho, self.sam_adaptive, self.sam_eta)
        if self.lr_schedule not in SCHEDULES:
            raise ValueError(f"unknown lr_schedule {self.lr_schedule!r} (choose from {SCHEDULES})")
        if self.lr_warmup_steps < 0 or self.lr_decay_steps < 0:
            raise ValueError("lr_warmup_steps and lr_decay_steps must be >= 0")
        if self.lr_schedule != "constant" and self.lr_decay_steps <= 0:
            raise ValueError(f"lr_schedule {self.lr_schedule!r} needs lr_decay_steps > 0 "
                             "(the worker defaults it to max_steps)")
        if self.adamw and not (0.0 < self.beta1 < 1.0 and 0.0 < self.beta2 < 1.0 and self.adam_eps > 0.0):
            raise ValueError("adamw needs 0 < beta1, beta2 < 1 and adam_eps > 0")
        if not self.clip_grad_norm >= 0.0:  # negative or NaN
            raise ValueError("clip_grad_norm must be >= 0 (0: off, inf: measure the norm only)")
        _ema_last(self.ema_decay, self.ema_warmup)  # a bad decay, a warm-up table that is too long

    @property
    def clips(self) -> bool:
        return self.clip_grad_norm > 0.0

    @property
    def agcs(self) -> bool:
        return self.agc_clip > 0.0

    @property
    def sams(self) -> bool:
        return self.sam_rho > 0.0

    @property
    def emas(self) -> bool:
        return self.ema_decay > 0.0

    def ema_table(self) -> np.ndarray | None:
        """:func:`ema_table` of this spec; None with the EMA off."""
        return ema_table(self.ema_decay, self.ema_warmup) if self.emas else None

    @property
    def adamw(self) -> bool:
        return self.optimizer == "adamw"

    @property
    def lars(self) -> bool:
        return self.optimizer == "lars"

    @property
    def muon(self) -> bool:
        return self.optimizer == "muon"

    @property
    def scheduled(self) -> bool:
        return self.lr_schedule != "constant" or self.lr_warmup_steps > 0

    @property
    def mapped(self) -> bool:
        """The update reads the class map: decay groups on, or LARS (whose exclusion list the
        classes are) or Muon (whose other elements follow the grouped rule), whether or not a class
        decay is set."""
        return self.grouped or self.lars or self.muon

    @property
    def grouped(self) -> bool:
        """Decay groups on: at least one of the two class decays is set."""
        return self.norm_weight_decay is not None or self.bias_weight_decay is not None

    def decays(self) -> tuple:
        """The effective decay of each class (:data:`DECAY_CLASSES`)."""
        wd = self.weight_decay
        return (wd, wd if self.norm_weight_decay is None else self.norm_weight_decay,
                wd if self.bias_weight_decay is None else self.bias_weight_decay)

    @property
    def plain(self) -> bool:
        """Momentum SGD at a fixed lr without decay groups: the rule without a step counter.  A
        grouped trainer always runs a step-counter rule (a grouped SGD trainer at a fixed lr runs
        ``RULE_SGD_LR`` with no table, which reads the scalar lr), so it has an ``opt_step``, and
        the plain rule's kernels and launches are what they were before groups existed.  Nor is a
        LARS or a Muon trainer ever plain."""
        return not self.adamw and not self.scheduled and not self.grouped and not self.lars and not self.muon

    @property
    def rule(self) -> int:
        return RULE_ADAMW if self.adamw else RULE_SGD if self.plain else RULE_SGD_LR

    def lr_at(self, step: int) -> float:
        return lr_at(step, self.lr, self.lr_schedule, self.lr_warmup_steps, self.lr_decay_steps, self.lr_min_ratio)

    def lr_table(self) -> np.ndarray | None:
        """fp32 ``lr_at`` of steps 0 .. last, where every later step has the last one's value
        (the kernels index it with ``min(step, last)``); None at a fixed lr."""
        if not self.scheduled:
            return None
        last = self.lr_warmup_steps
        if self.lr_schedule != "constant":
            last = max(self.lr_decay_steps, self.lr_warmup_steps + 1)
        return np.array([self.lr_at(s) for s in range(last + 1)], dtype=np.float32)

    def adam_scalars(self) -> tuple:
        """The kernels' beta-derived scalars, each computed in double and rounded once (fp32
        ``1 - 0.999`` is 3e-5 off; ``1 - beta^t`` is ``-expm1(t ln beta)`` on the device)."""
        if not self.adamw:
            return (0.0,) * 7
        return (self.beta1, self.beta2, 1.0 - self.beta1, 1.0 - self.beta2, math.log(self.beta1),
                math.log(self.beta2), self.adam_eps)

    def update(self, flat, mom, v, grad, step: int, decay=None, plan=None):
        """One reference update of 0-based ``step``, in place (the CPU trainers' optimizer).
        ``decay``: the per-element weight decay of a grouped spec (:func:`decay_vector`).
        ``plan``: the :func:`lars_plan` of a LARS spec, which takes the class decays from
        :meth:`decays` and returns :func:`lars_update`'s ``(wn, gn, trust)`` rows; or the
        :func:`muon_plan` of a Muon spec, which returns :func:`muon_update`'s norms."""
        if self.muon:
            assert plan is not None, "a Muon spec updates with its plan"
            return muon_update(flat, mom, grad, self.lr_at(step), self.momentum, self.decays(), plan,
                               self.muon_lr_ratio, self.muon_nesterov, self.muon_ns_steps)
        if self.lars:
            assert plan is not None, "a LARS spec updates with its plan"
            return lars_update(flat, mom, grad, self.lr_at(step), self.momentum, self.decays(), plan,
                               self.lars_eta, self.lars_eps)
        assert (decay is not None) == self.grouped, "a grouped spec updates with its decay vector"
        wd = self.weight_decay if decay is None else decay
        if self.adamw:
            adamw_update(flat, mom, v, grad, self.lr_at(step), self.beta1, self.beta2, self.adam_eps, wd, step + 1)
        else:
            sgd_update(flat, mom, grad, self.lr_at(step), self.momentum, wd)

    def meta(self) -> dict:
        """Checkpoint metadata (``meta["optimizer"]``)."""
        d = {"lr": self.lr, "momentum": self.momentum}
        if not self.plain:
            d.update(name=self.optimizer, beta1=self.beta1, beta2=self.beta2, eps=self.adam_eps,
                     weight_decay=self.weight_decay, schedule=self.lr_schedule, warmup_steps=self.lr_warmup_steps,
                     decay_steps=self.lr_decay_steps, min_ratio=self.lr_min_ratio)
        if self.clips:
            d["clip_grad_norm"] = self.clip_grad_norm
        if self.emas:
            d.update(ema_decay=self.ema_decay, ema_warmup=bool(self.ema_warmup))
        if self.norm_weight_decay is not None:
            d["norm_weight_decay"] = self.norm_weight_decay
        if self.bias_weight_decay is not None:
            d["bias_weight_decay"] = self.bias_weight_decay
        if self.lars:
            d.update(lars_eta=self.lars_eta, lars_eps=self.lars_eps)
        if self.muon:
            d.update(muon_lr_ratio=self.muon_lr_ratio, muon_nesterov=bool(self.muon_nesterov),
                     muon_ns_steps=int(self.muon_ns_steps))
        if self.agcs:
            d.update(agc_clip=self.agc_clip, agc_eps=self.agc_eps)
        if self.sams:
            d.update(sam_rho=self.sam_rho, sam_adaptive=bool(self.sam_adaptive), sam_eta=self.sam_eta)
        return d


def require_kernels(spec: OptSpec, *names: str) -> None:
    """The step-counter rules, gradient clipping, gradient accumulation and the weight EMA need
    their entry points: an older kernel build (kept for A/B runs of the SGD path) does not have them, and
    there is no fallback."""
    lib = N.lib()
    missing = [n for n in names if not hasattr(lib, n)]
    if missing:
        raise RuntimeError(f"optimizer {spec.optimizer!r} / lr_schedule {spec.lr_schedule!r} / clip_grad_norm "
                           f"{spec.clip_grad_norm!r} / accum_steps > 1 / ema_decay {spec.ema_decay!r} / decay groups "
                           f"{'on' if spec.grouped else 'off'} need {', '.join(missing)}: not in this kernel library")


# ---- flat kernels ----
def _check_flat(w, g, shadow):
    assert w.is_cuda and w.dtype == torch.float32 and g.dtype == torch.float32
    assert w.is_contiguous() and g.is_contiguous() and g.numel() == w.numel()
    if shadow is not None:
        assert shadow.dtype == torch.bfloat16 and shadow.numel() == w.numel()


def sgd_flat(w: torch.Tensor, g: torch.Tensor, mom: torch.Tensor | None, lr: float, momentum: float = 0.0,
             weight_decay: float = 0.0, shadow: torch.Tensor | None = None, grad_scale: float = 1.0) -> None:
    _check_flat(w, g, shadow)
    N.call("sl_sgd_flat", N.ptr(w), N.ptr(g), N.ptr(mom), N.ptr(shadow), w.numel(), float(lr), float(momentum),
           float(weight_decay), float(grad_scale), N.stream_ptr())


def sgd_flat_lr(w: torch.Tensor, g: torch.Tensor, mom: torch.Tensor | None, step: torch.Tensor,
                lr_tab: torch.Tensor, momentum: float = 0.0, weight_decay: float = 0.0,
                shadow: torch.Tensor | None = None, grad_scale: float = 1.0) -> None:
    """sgd_flat at the learning rate ``lr_tab[min(step, len - 1)]`` (``step``: int32 on the device)."""
    _check_flat(w, g, shadow)
    assert step.dtype == torch.int32 and lr_tab.dtype == torch.float32
    N.call("sl_sgd_flat_lr", N.ptr(w), N.ptr(g), N.ptr(mom), N.ptr(shadow), w.numel(), N.ptr(step), N.ptr(lr_tab),
           lr_tab.numel(), float(momentum), float(weight_decay), float(grad_scale), N.stream_ptr())


def adamw_flat(w: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: torch.Tensor,
               spec: OptSpec, lr_tab: torch.Tensor | None = None, shadow: torch.Tensor | None = None,
               grad_scale: float = 1.0) -> None:
    """One AdamW update of step ``step`` (int32 on the device; the caller advances it)."""
    _check_flat(w, g, shadow)
    assert step.dtype == torch.int32 and m.numel() == w.numel() and v.numel() == w.numel()
    N.call("sl_adamw_flat", N.ptr(w), N.ptr(g), N.ptr(m), N.ptr(v), N.ptr(shadow), w.numel(), N.ptr(step),
           N.ptr(lr_tab), lr_tab.numel() if lr_tab is not None else 0, float(spec.lr), float(spec.weight_decay),
           float(grad_scale), *spec.adam_scalars(), N.stream_ptr())


FLAT_GROUP_KERNELS = ("sl_adamw_flat_groups", "sl_sgd_flat_lr_groups")


def _check_cls(cls: torch.Tensor, n: int) -> None:
    assert cls.is_cuda and cls.dtype == torch.uint8 and cls.is_contiguous()
    assert cls.numel() * DECAY_BLOCK >= n, "the class map is shorter than the vector"


def sgd_flat_lr_groups(w: torch.Tensor, g: torch.Tensor, mom: torch.Tensor | None, step: torch.Tensor,
                       lr_tab: torch.Tensor | None, cls: torch.Tensor, decays, lr: float = 0.0, momentum: float = 0.0,
                       shadow: torch.Tensor | None = None, grad_scale: float = 1.0) -> None:
    """:func:`sgd_flat_lr` with the weight decay ``decays[cls[i // 64]]`` for element ``i`` (``cls``:
    uint8 on the device, :func:`decay_class_map`); without a table the learning rate is ``lr``."""
    _check_flat(w, g, shadow)
    _check_cls(cls, w.numel())
    assert step.dtype == torch.int32 and (lr_tab is None or lr_tab.dtype == torch.float32)
    wd, wd_norm, wd_bias = (float(d) for d in decays)
    N.call("sl_sgd_flat_lr_groups", N.ptr(w), N.ptr(g), N.ptr(mom), N.ptr(shadow), w.numel(), N.ptr(step),
           N.ptr(lr_tab), lr_tab.numel() if lr_tab is not None else 0, float(lr), float(momentum), wd,
           float(grad_scale), N.ptr(cls), wd_norm, wd_bias, N.stream_ptr())


def adamw_flat_groups(w: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: torch.Tensor,
                      spec: OptSpec, cls: torch.Tensor, lr_tab: torch.Tensor | None = None,
                      shadow: torch.Tensor | None = None, grad_scale: float = 1.0) -> None:
    """:func:`adamw_flat` with the weight decay ``spec.decays()[cls[i // 64]]`` for element ``i``."""
    _check_flat(w, g, shadow)
    _check_cls(cls, w.numel())
    assert step.dtype == torch.int32 and m.numel() == w.numel() and v.numel() == w.numel()
    wd, wd_norm, wd_bias = (float(d) for d in spec.decays())
    N.call("sl_adamw_flat_groups", N.ptr(w), N.ptr(g), N.ptr(m), N.ptr(v), N.ptr(shadow), w.numel(), N.ptr(step),
           N.ptr(lr_tab), lr_tab.numel() if lr_tab is not None else 0, float(spec.lr), wd, float(grad_scale),
           *spec.adam_scalars(), N.ptr(cls), wd_norm, wd_bias, N.stream_ptr())


LARS_KERNELS = ("sl_lars_chunk", "sl_lars_norms", "sl_lars_trust", "sl_sgd_flat_lars")


class LarsBuffers:
    """A :class:`LarsPlan` on a device, uploaded once: the chunk and tensor tables, the block map
    and the class map, and what the launches write, ``partials`` (fp64 ``[C][2]``) and ``out``
    (fp32 ``[T][3]`` = (wn, gn, trust) of the last update)."""

    def __init__(self, plan: LarsPlan, device):
        assert int(N.lib().sl_lars_chunk()) == LARS_CHUNK, "the kernel library was built with another LARS_CHUNK"
        up = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
        self.plan = plan
        self.chunks, self.tensors = up(plan.chunks), up(plan.tensors)
        # (torch has no uint16 arithmetic, and needs none: the map is only handed to the kernel)
        self.block_map = up(plan.block_map.view(np.int16))
        self.cls = up(plan.cls)
        self.partials = torch.zeros(len(plan.chunks), 2, dtype=torch.float64, device=device)
        self.out = torch.zeros(len(plan.names), 3, dtype=torch.float32, device=device)

    def ratios(self) -> dict:
        """``{tensor name: (wn, gn, trust)}`` of the last update (one read from the device)."""
        return {name: tuple(row) for name, row in zip(self.plan.names, self.out.tolist())}


def _check_lars(w: torch.Tensor, g: torch.Tensor, b: LarsBuffers) -> None:
    assert w.is_cuda and w.dtype == torch.float32 and g.dtype == torch.float32
    assert w.is_contiguous() and g.is_contiguous() and g.numel() == w.numel()
    assert w.numel() == b.plan.n, "the plan was made for a vector of another length"  # (every chunk is inside it)
    assert b.chunks.device == w.device


def lars_norms(w: torch.Tensor, g: torch.Tensor, b: LarsBuffers) -> None:
    """``b.partials[c] = (sum w^2, sum g^2)`` over chunk ``c`` of the plan: one launch, one
    workgroup per chunk, fp64 sums in a fixed order (csrc/kernels/lars.hip lars_norms_kernel)."""
    _check_lars(w, g, b)
    N.call("sl_lars_norms", N.ptr(w), N.ptr(g), N.ptr(b.chunks), b.chunks.shape[0], N.ptr(b.partials), N.stream_ptr())


def lars_trust(b: LarsBuffers, eta: float, eps: float, weight_decay: float) -> None:
    """``b.out[t] = (wn, gn, trust)`` of every adapted tensor from ``b.partials``: one wave per
    tensor, formed in fp64 and rounded once (lars_trust_kernel)."""
    N.call("sl_lars_trust", N.ptr(b.partials), N.ptr(b.tensors), b.tensors.shape[0], float(eta), float(eps),
           float(weight_decay), N.ptr(b.out), N.stream_ptr())


def sgd_flat_lars(w: torch.Tensor, g: torch.Tensor, mom: torch.Tensor | None, step: torch.Tensor,
                  lr_tab: torch.Tensor | None, b: LarsBuffers, decays, lr: float = 0.0, momentum: float = 0.0,
                  shadow: torch.Tensor | None = None) -> None:
    """The LARS update launch (lars_update_kernel): :func:`sgd_flat_lr_groups` with the decayed
    gradient of element ``i`` scaled by ``b.out[b.block_map[i // 64]]``'s trust (1 where no tensor
    owns the block).  The caller advances ``step``."""
    _check_flat(w, g, shadow)
    _check_lars(w, g, b)
    assert step.dtype == torch.int32 and (lr_tab is None or lr_tab.dtype == torch.float32)
    assert mom is None or (mom.dtype == torch.float32 and mom.numel() == w.numel())
    wd, wd_norm, wd_bias = (float(d) for d in decays)
    N.call("sl_sgd_flat_lars", N.ptr(w), N.ptr(g), N.ptr(mom), N.ptr(shadow), w.numel(), N.ptr(step), N.ptr(lr_tab),
           lr_tab.numel() if lr_tab is not None else 0, float(lr), float(momentum), wd, wd_norm, wd_bias,
           N.ptr(b.cls), N.ptr(b.block_map), N.ptr(b.out), b.tensors.shape[0], N.stream_ptr())


MUON_KERNELS = ("sl_muon_chunk", "sl_muon_prep", "sl_muon_gram", "sl_muon_poly", "sl_muon_apply", "sl_sgd_flat_muon")


class MuonBuffers:
    """A :class:`MuonPlan` on a device, uploaded once, with the work buffers the launches share:
    ``x`` (two bf16 copies of the Muon tensors, the iteration's ping and pong), ``a`` and ``b`` (the
    Gram matrix and its polynomial), ``ws`` (the fp32 split-K partials of the Gram launch),
    ``partials`` (fp64 per chunk) and ``norms`` (fp32 ``||u||_F`` per tensor, of the last update)."""

    def __init__(self, plan: MuonPlan, device):
        assert int(N.lib().sl_muon_chunk()) == MUON_CHUNK, "the kernel library was built with another MUON_CHUNK"
        up = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
        zeros = lambda k, dt: torch.zeros(k, dtype=dt, device=device)  # noqa: E731
        self.plan, self.T = plan, len(plan.names)
        self.tensors_h = np.ascontiguousarray(plan.tensors)  # (the launchers check the shapes on the host copy)
        self.tensors, self.chunks = up(plan.tensors), up(plan.chunks)
        self.tiles, self.gram_tiles, self.tri_tiles, self.poly_tiles = (
            up(t) for t in (plan.tiles, plan.gram_tiles, plan.tri_tiles, plan.poly_tiles))
        self.block_map, self.cls = up(plan.block_map.view(np.int16)), up(plan.cls)
        self.x = (zeros(plan.x_elems, torch.bfloat16), zeros(plan.x_elems, torch.bfloat16))
        self.a, self.b = zeros(plan.a_elems, torch.bfloat16), zeros(plan.a_elems, torch.bfloat16)
        self.ws = zeros(plan.ws_floats, torch.float32)
        self.partials = zeros(len(plan.chunks), torch.float64)
        self.norms = zeros(self.T, torch.float32)

    def _tab(self) -> tuple:
        return self.tensors_h.ctypes.data, N.ptr(self.tensors), self.T

    def out(self, ns_steps: int) -> torch.Tensor:
        """The work buffer that holds O after ``ns_steps`` iterations."""
        return self.x[ns_steps & 1]

    def matrix(self, t: int, ns_steps: int) -> torch.Tensor:
        """O of tensor ``t`` as its own ``[m][n]``, on the device (a tall one transposed back)."""
        off, m, k, tall, xoff = self.plan.tensors[t, :5].tolist()
        o = self.out(ns_steps)[xoff:xoff + m * k]
        return o.view(k, m).T if tall else o.view(m, k)


def _check_muon(g: torch.Tensor, mom: torch.Tensor, b: MuonBuffers) -> None:
    assert g.is_cuda and g.dtype == torch.float32 and mom.dtype == torch.float32
    assert g.is_contiguous() and mom.is_contiguous() and g.numel() == mom.numel()
    assert g.numel() == b.plan.n, "the plan was made for a vector of another length"  # (every chunk is inside it)
    assert b.tensors.device == g.device


def muon_prep(g: torch.Tensor, mom: torch.Tensor, b: MuonBuffers, momentum: float, nesterov: bool = True) -> None:
    """The Muon tensors' ``mom = fma(mu, mom, g)``, their ``||u||_F`` into ``b.norms`` and their
    scaled bf16 ``X0`` into ``b.x[0]`` (muon_mom_kernel, muon_x0_kernel)."""
    _check_muon(g, mom, b)
    N.call("sl_muon_prep", N.ptr(g), N.ptr(mom), N.ptr(b.chunks), b.chunks.numel(), float(momentum), int(bool(nesterov)),
           N.ptr(b.partials), *b._tab(), N.ptr(b.tiles), b.tiles.shape[0], N.ptr(b.x[0]), N.ptr(b.norms),
           N.stream_ptr())


def muon_gram(b: MuonBuffers, k: int) -> None:
    """``b.a = bf16(X X^T)`` of iteration ``k``'s X, ``b.x[k & 1]`` (muon_gram_kernel, muon_fold_kernel)."""
    N.call("sl_muon_gram", N.ptr(b.x[k & 1]), *b._tab(), N.ptr(b.gram_tiles), b.gram_tiles.shape[0], N.ptr(b.ws),
           N.ptr(b.tri_tiles), b.tri_tiles.shape[0], N.ptr(b.a), N.stream_ptr())


def muon_poly(b: MuonBuffers) -> None:
    """``b.b = bf16(b A + c A A)`` (muon_poly_kernel)."""
    N.call("sl_muon_poly", N.ptr(b.a), *b._tab(), N.ptr(b.poly_tiles), b.poly_tiles.shape[0], N.ptr(b.b),
           N.stream_ptr())


def muon_apply(b: MuonBuffers, k: int) -> None:
    """``b.x[(k + 1) & 1] = bf16(a X + B X)`` of iteration ``k``'s X (muon_apply_kernel)."""
    N.call("sl_muon_apply", N.ptr(b.x[k & 1]), N.ptr(b.b), *b._tab(), N.ptr(b.tiles), b.tiles.shape[0],
           N.ptr(b.x[(k + 1) & 1]), N.stream_ptr())


def muon_orthogonalize(g: torch.Tensor, mom: torch.Tensor, b: MuonBuffers, momentum: float, nesterov: bool = True,
                       ns_steps: int = 5) -> None:
    """Prep and ``ns_steps`` x (gram, poly, apply): ``b.out(ns_steps)`` then holds every O."""
    muon_prep(g, mom, b, momentum, nesterov)
    for k in range(int(ns_steps)):
        muon_gram(b, k)
        muon_poly(b)
        muon_apply(b, k)


def sgd_flat_muon(w: torch.Tensor, g: torch.Tensor, mom: torch.Tensor, step: torch.Tensor,
                  lr_tab: torch.Tensor | None, b: MuonBuffers, decays, lr: float = 0.0, momentum: float = 0.0,
                  lr_ratio: float = 1.0, ns_steps: int = 5, shadow: torch.Tensor | None = None) -> None:
    """The Muon update launch (muon_update_kernel): the blocks ``b.block_map`` gives to a Muon
    tensor take ``w = w (1 - lr r wd) - lr r s_T O`` with O from ``b.out(ns_steps)``; every other
    element is :func:`sgd_flat_lr_groups`'s, bit for bit.  The caller advances ``step``."""
    _check_flat(w, g, shadow)
    _check_muon(g, mom, b)
    assert step.dtype == torch.int32 and (lr_tab is None or lr_tab.dtype == torch.float32)
    wd, wd_norm, wd_bias = (float(d) for d in decays)
    N.call("sl_sgd_flat_muon", N.ptr(w), N.ptr(g), N.ptr(mom), N.ptr(shadow), w.numel(), N.ptr(step), N.ptr(lr_tab),
           lr_tab.numel() if lr_tab is not None else 0, float(lr), float(momentum), wd, wd_norm, wd_bias, 1.0,
           float(lr_ratio), N.ptr(b.cls), N.ptr(b.block_map), *b._tab(), N.ptr(b.x[0]), N.ptr(b.x[1]), int(ns_steps),
           N.stream_ptr())


AGC_KERNELS = ("sl_agc_clip",)


class AgcBuffers:
    """An :class:`AgcPlan` on a device, uploaded once (the launcher checks the tables' host copies),
    and what the launch writes: ``stats``, fp32 ``[U][3]`` = (wn, gn, s) of the last call in the
    plan's order, ``s = 1`` for a unit it left alone."""

    def __init__(self, plan: AgcPlan, device):
        self.plan = plan
        self.units_h, self.work_h = np.ascontiguousarray(plan.units), np.ascontiguousarray(plan.work)
        self.units, self.work = torch.from_numpy(self.units_h).to(device), torch.from_numpy(self.work_h).to(device)
        self.stats = torch.zeros(len(plan.units), 3, dtype=torch.float32, device=device)


def agc_clip_flat(w: torch.Tensor, g: torch.Tensor, b: AgcBuffers, clip: float, eps: float = 1e-3) -> None:
    """:func:`agc_clip_reference` on the device, in place on ``g``, in one grouped launch
    (csrc/kernels/agc.hip): one wave per unit, the gradient row in registers from its load to its
    store, both norms in fp64 by the same two passes, a unit that is not clipped not written.
    ``b.stats`` receives every unit's ``(wn, gn, s)``.  No host synchronisation and no state between
    calls, so a captured graph replays it; bit-identical from call to call and in both builds."""
    assert w.is_cuda and w.dtype == torch.float32 and g.dtype == torch.float32
    assert w.is_contiguous() and g.is_contiguous() and g.numel() == w.numel()
    assert w.numel() >= b.plan.n and b.units.device == w.device
    N.call("sl_agc_clip", N.ptr(w), N.ptr(g), w.numel(), b.units_h.ctypes.data, N.ptr(b.units), len(b.units_h),
           b.work_h.ctypes.data, N.ptr(b.work), len(b.work_h), float(clip), float(eps), N.ptr(b.stats),
           N.stream_ptr())


SAM_KERNELS = ("sl_sam_chunk", "sl_sam_norms", "sl_sam_scale", "sl_sam_perturb", "sl_accum_flat")


class SamBuffers:
    """What a SAM step keeps on a device for a vector of ``n`` elements (a multiple of 64) with the class
    map ``cls``: the map, ``partials`` (one fp64 sum per :data:`SAM_CHUNK` elements), ``out`` (fp64 ``(nrm,
    scale)`` of the last perturbation) and ``saved`` (the unperturbed weights, the way back)."""

    def __init__(self, cls: np.ndarray, n: int, device):
        assert int(N.lib().sl_sam_chunk()) == SAM_CHUNK, "the kernel library was built with another SAM_CHUNK"
        assert n > 0 and n % DECAY_BLOCK == 0 and len(cls) * DECAY_BLOCK == n, "whole class blocks"
        self.n = int(n)
        self.cls = torch.from_numpy(np.ascontiguousarray(cls, dtype=np.uint8)).to(device)
        self.partials = torch.zeros((self.n + SAM_CHUNK - 1) // SAM_CHUNK, dtype=torch.float64, device=device)
        self.out = torch.zeros(2, dtype=torch.float64, device=device)
        self.saved = torch.zeros(self.n, dtype=torch.float32, device=device)


def _check_sam(w: torch.Tensor, g: torch.Tensor, b: SamBuffers) -> None:
    assert w.is_cuda and w.dtype == torch.float32 and g.dtype == torch.float32
    assert w.is_contiguous() and g.is_contiguous() and g.numel() == w.numel()
    assert w.numel() == b.n and b.cls.device == w.device, "the buffers were made for another vector"


def sam_norms(w: torch.Tensor, g: torch.Tensor, b: SamBuffers, adaptive: bool = False, eta: float = 0.01) -> None:
    """``b.partials[c]`` = the sum of ``(T_i g_i)^2`` over chunk ``c``: one launch, one workgroup per chunk,
    fp64 products and sums in a fixed order (csrc/kernels/sam.hip sam_norms_kernel)."""
    _check_sam(w, g, b)
    N.call("sl_sam_norms", N.ptr(w), N.ptr(g), N.ptr(b.cls), b.n, int(bool(adaptive)), float(eta), N.ptr(b.partials),
           b.partials.numel(), N.stream_ptr())


def sam_scale(b: SamBuffers, rho: float) -> None:
    """``b.out = (nrm, scale)`` from ``b.partials``, folded in chunk order by one wave (sam_scale_kernel)."""
    N.call("sl_sam_scale", N.ptr(b.partials), b.partials.numel(), float(rho), N.ptr(b.out), N.stream_ptr())


def sam_perturb(w: torch.Tensor, g: torch.Tensor, shadow: torch.Tensor, b: SamBuffers, adaptive: bool = False,
                eta: float = 0.01) -> None:
    """``b.saved = w``, ``w = w'`` and ``shadow = bf16(w')`` with ``b.out``'s scale, in one launch
    (sam_perturb_kernel); :func:`sam_restore` undoes it."""
    _check_sam(w, g, b)
    assert shadow.dtype == torch.bfloat16 and shadow.numel() == w.numel() and shadow.is_contiguous()
    N.call("sl_sam_perturb", N.ptr(w), N.ptr(g), N.ptr(b.saved), N.ptr(shadow), b.n, N.ptr(b.cls), int(bool(adaptive)),
           float(eta), N.ptr(b.out), N.stream_ptr())


def sam_restore(w: torch.Tensor, b: SamBuffers) -> None:
    """``w = b.saved``: a copy (:func:`accum_flat`, ``add`` off), so the weights return bit for bit."""
    accum_flat(w, b.saved, False)


def to_bf16(src: torch.Tensor, dst: torch.Tensor) -> None:
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and src.numel() == dst.numel()
    N.call("sl_to_bf16", N.ptr(src), N.ptr(dst), src.numel(), N.stream_ptr())


CLIP_KERNELS = ("sl_clip_grad_norm", "sl_clip_grad_partials")


def clip_partials(n: int) -> int:
    """fp64 partials :func:`clip_grad_norm_flat` needs for a vector of ``n`` floats."""
    return int(N.lib().sl_clip_grad_partials(int(n)))


def clip_buffers(n: int, device) -> tuple:
    """(partials, norm_out) for clipping a vector of ``n`` floats on ``device``."""
    return (torch.zeros(max(1, clip_partials(n)), dtype=torch.float64, device=device),
            torch.zeros(1, dtype=torch.float32, device=device))


def clip_grad_norm_flat(g: torch.Tensor, max_norm: float, partials: torch.Tensor, norm_out: torch.Tensor) -> None:
    """:func:`clip_grad_` on the device, in place, in two launches (csrc/kernels/elementwise.hip):
    ``norm_out[0]`` receives the norm before clipping.  No host synchronisation and no state
    between calls, so a captured graph replays it; bit-identical from call to call."""
    assert g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()
    assert partials.dtype == torch.float64 and partials.is_contiguous() and norm_out.dtype == torch.float32
    N.call("sl_clip_grad_norm", N.ptr(g), g.numel(), float(max_norm), N.ptr(partials), partials.numel(),
           N.ptr(norm_out), N.stream_ptr())


ACCUM_KERNELS = ("sl_accum_flat",)


def check_accum_steps(k) -> int:
    """``accum_steps`` of a trainer: an integer >= 1."""
    if isinstance(k, bool) or int(k) != k or int(k) < 1:
        raise ValueError(f"accum_steps must be an integer >= 1, got {k!r}")
    return int(k)


def accum_flat(dst: torch.Tensor, src: torch.Tensor, add) -> None:
    """Gradient accumulation's one launch (csrc/kernels/elementwise.hip): ``dst = dst + src``
    (``add``) or ``dst = src``, elementwise in fp32, one rounding per element and no atomics, so
    the bits are the same from call to call and in both kernel builds.  ``dst`` and ``src`` are
    contiguous fp32 ranges of one length that do not overlap; any 4-byte alignment will do (views
    ``grad[lo:hi]`` of the flat vector)."""
    assert dst.is_cuda and src.is_cuda and dst.dtype == torch.float32 and src.dtype == torch.float32
    assert dst.is_contiguous() and src.is_contiguous() and dst.numel() == src.numel()
    nbytes, a, b = 4 * dst.numel(), dst.data_ptr(), src.data_ptr()
    assert a + nbytes <= b or b + nbytes <= a, "accum_flat: dst and src overlap"
    N.call("sl_accum_flat", a, b, dst.numel(), int(bool(add)), N.stream_ptr())


EMA_KERNELS = ("sl_ema_flat",)


def ema_flat(ema: torch.Tensor, w: torch.Tensor, step: torch.Tensor, ticket: torch.Tensor, tab: torch.Tensor) -> None:
    """:func:`ema_update_` on the device in one launch (csrc/kernels/elementwise.hip): ``ema +=
    tab[min(step, len - 1)] * (w - ema)`` in three fp32 roundings, then ``step += 1`` (``step``:
    int32 on the device; ``ticket``: a zeroed int32 word the launch uses to find its last workgroup
    and leaves at zero).  No host synchronisation, so a captured graph replays it with a moving
    coefficient; the same bits from call to call and in both kernel builds.  ``ema`` and ``w`` are
    whole 16-byte-aligned fp32 vectors of one length that do not overlap."""
    assert ema.is_cuda and w.is_cuda and ema.dtype == torch.float32 and w.dtype == torch.float32
    assert ema.is_contiguous() and w.is_contiguous() and ema.numel() == w.numel()
    assert step.dtype == torch.int32 and ticket.dtype == torch.int32 and step.numel() == 1 and ticket.numel() == 1
    assert tab.dtype == torch.float32 and tab.is_contiguous() and tab.numel() >= 1
    nbytes, a, b = 4 * ema.numel(), ema.data_ptr(), w.data_ptr()
    assert a + nbytes <= b or b + nbytes <= a, "ema_flat: ema and w overlap"
    N.call("sl_ema_flat", a, b, ema.numel(), N.ptr(step), N.ptr(ticket), N.ptr(tab), tab.numel(), N.stream_ptr())
