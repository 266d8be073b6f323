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

OPTIMIZERS = ("sgd", "adamw")
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


CLIP_EPS = 1e-6  # torch.nn.utils.clip_grad_norm_'s constant


def clip_grad_(g: torch.Tensor, max_norm: float) -> float:
    """``torch.nn.utils.clip_grad_norm_`` over one flat gradient, in place: with ``total`` the
    L2 norm of ``g`` (taken in float64), ``g *= min(1, max_norm / (total + 1e-6))``.  Returns
    ``total``, the norm before clipping; ``max_norm = inf`` measures and never scales."""
    total = float(torch.linalg.vector_norm(g.detach().double()))
    coef = min(1.0, float(max_norm) / (total + CLIP_EPS))
    g.mul_(coef)
    return total


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

    def __post_init__(self):
        check_group_decay("norm_weight_decay", self.norm_weight_decay)
        check_group_decay("bias_weight_decay", self.bias_weight_decay)
        if self.optimizer not in OPTIMIZERS:
            raise ValueError(f"unknown optimizer {self.optimizer!r} (choose from {OPTIMIZERS})")
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
    def emas(self) -> bool:
        return self.ema_decay > 0.0

    def ema_table(self) -> np.ndarray | None:
        """:func:`ema_table` of this spec; None with the EMA off."""
        return ema_table(self.ema_decay, self.ema_warmup) if self.emas else None

    @property
    def adamw(self) -> bool:
        return self.optimizer == "adamw"

    @property
    def scheduled(self) -> bool:
        return self.lr_schedule != "constant" or self.lr_warmup_steps > 0

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
        the plain rule's kernels and launches are what they were before groups existed."""
        return not self.adamw and not self.scheduled and not self.grouped

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

    def update(self, flat, mom, v, grad, step: int, decay=None) -> None:
        """One reference update of 0-based ``step``, in place (the CPU trainers' optimizer).
        ``decay``: the per-element weight decay of a grouped spec (:func:`decay_vector`)."""
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
