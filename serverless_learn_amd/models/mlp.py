"""The flagship model: a 3-layer MLP (784-256-256-10) on MNIST-shaped data.

The reference has no model at all -- its "model" is a ``std::vector<double>``
that ``simulate_training`` bumps by one every 2 s
(/root/reference/src/worker.cc:221-231) and that workers mix by gossip
(/root/reference/src/worker.cc:81-100).  This module provides the real model
that takes its place, in three forms:

* :func:`param_layout` / :func:`init_params` -- the flat fp32 parameter vector.
  A flat vector is what travels in the reference's ``Update{repeated double
  delta}`` message (proto :81-83), what the checkpoint format stores and what
  the data-parallel all-reduce moves in one bucket.
* :class:`MLP` -- a ``torch.nn.Module`` view of that vector, used on CPU
  workers (BASELINE config 1, "plumbing, no GPU") and as the fp32 reference
  in numerics tests.
* :class:`FusedMLPTrainer` -- the MI355X path: three hand-written HIP kernels
  per step (csrc/kernels/mlp_fused.hip) on bf16 MFMA with fp32 master
  weights, optionally wrapped in a hipGraph, with an RCCL all-reduce hook.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

# (the rules' semantics live there)
from ..ops.optim import (OptSpec, adamw_update, check_accum_steps, clip_grad_, ema_update_, lr_at,  # noqa: F401
                         sgd_update)
from ..utils.graphs import GraphSlots

D_IN = 784
D_IN_PAD = 832  # w1h row stride: layer-1 K in 13 chunks of 64 (mlp_fused.hip)
HIDDEN = 256
CLASSES = 10
MNIST_MEAN = 0.1307
MNIST_STD = 0.3081
BLOCK_ROWS = 64  # batch rows per workgroup of the fused row kernel
W3P_LD = 3088  # row stride of the rows kernel's partial rows: [dW3 | db3 | pad | db1 | db2]
R1_BLK = 25  # 32-column blocks per W1 row: fixed-point partial row sums of the fp16 shadow
R1_OVF_MIN = 1 << 51  # a partial row sum at or past this flags a W1 weight beyond fp16 (mlp_fused.hip)

LAYOUT = (
    ("fc1.weight", (HIDDEN, D_IN)),
    ("fc1.bias", (HIDDEN,)),
    ("fc2.weight", (HIDDEN, HIDDEN)),
    ("fc2.bias", (HIDDEN,)),
    ("fc3.weight", (CLASSES, HIDDEN)),
    ("fc3.bias", (CLASSES,)),
)


def param_layout():
    """[(name, shape, offset, numel)] of the flat parameter vector."""
    out, off = [], 0
    for name, shape in LAYOUT:
        n = math.prod(shape)
        out.append((name, shape, off, n))
        off += n
    return out


N_PARAMS = sum(math.prod(s) for _, s in LAYOUT)  # 269,322
N_PARAMS_B1 = HIDDEN * D_IN  # offset of fc1.bias in the flat vector


def norm_coeffs(mean: float = MNIST_MEAN, std: float = MNIST_STD) -> tuple[float, float]:
    """u8 pixel p -> (p/255 - mean)/std == p*a + b."""
    return 1.0 / (255.0 * std), -mean / std


def init_params(seed: int = 0, device="cpu") -> torch.Tensor:
    """nn.Linear default init (U(-1/sqrt(fan_in), 1/sqrt(fan_in))) into a flat fp32 vector."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.empty(N_PARAMS, dtype=torch.float32)
    for name, shape, off, n in param_layout():
        fan_in = shape[1] if len(shape) == 2 else (D_IN if name.startswith("fc1") else HIDDEN)
        bound = 1.0 / math.sqrt(fan_in)
        flat[off:off + n] = (torch.rand(n, generator=g) * 2 - 1) * bound
    return flat.to(device)


def views(flat: torch.Tensor) -> dict:
    return {name: flat[off:off + n].view(shape) for name, shape, off, n in param_layout()}


def normalize(x_u8: torch.Tensor) -> torch.Tensor:
    a, b = norm_coeffs()
    return x_u8.float() * a + b


class MLP(nn.Module):
    """nn.Module over a flat parameter vector (CPU path and fp32 reference)."""

    def __init__(self, flat: torch.Tensor | None = None, seed: int = 0):
        super().__init__()
        if flat is None:
            flat = init_params(seed)
        self.flat = nn.Parameter(flat.clone().float())

    def forward(self, x_u8: torch.Tensor) -> torch.Tensor:
        v = views(self.flat)
        h = normalize(x_u8.reshape(-1, D_IN))
        h = F.relu(F.linear(h, v["fc1.weight"], v["fc1.bias"]))
        h = F.relu(F.linear(h, v["fc2.weight"], v["fc2.bias"]))
        return F.linear(h, v["fc3.weight"], v["fc3.bias"])


def reference_grads(flat: torch.Tensor, x_u8: torch.Tensor, y: torch.Tensor,
                    grad_scale: float | None = None):
    """fp32 autograd reference: (loss_sum, correct, grad_flat) with dZ scaled by grad_scale."""
    w = flat.detach().clone().float().requires_grad_(True)
    m = MLP.__new__(MLP)
    nn.Module.__init__(m)
    m.flat = w
    logits = m(x_u8)
    losses = F.cross_entropy(logits, y.long(), reduction="none")
    scale = grad_scale if grad_scale is not None else 1.0 / x_u8.shape[0]
    (losses.sum() * scale).backward()
    correct = (logits.argmax(1) == y.long()).float().sum()
    return losses.detach().sum(), correct.detach(), w.grad.detach()


def reference_grads_bf16(flat: torch.Tensor, x_u8: torch.Tensor, y: torch.Tensor, grad_scale: float):
    """fp32 math with bf16 rounding at exactly the points the fused kernels round.

    A tight check of csrc/kernels/mlp_fused.hip: any indexing/layout bug shows
    up as an O(1) error, while legitimate differences are fp32 summation order.
    Returns (loss_sum, correct, grad_flat).
    """
    r = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    v = {k: t.detach().float() for k, t in views(flat).items()}
    a, b = norm_coeffs()
    # layer 1: exact normalised pixels against the fp16 W1 shadow (the kernel multiplies the
    # exact pixels 1024 + u and removes the offset with W1's exact row sums)
    xe = x_u8.reshape(-1, D_IN).float() * a + b
    w1 = v["fc1.weight"].to(torch.float16).float()
    w2, w3 = r(v["fc2.weight"]), r(v["fc3.weight"])
    p1 = xe @ w1.t() + v["fc1.bias"]
    h1 = r(torch.relu(p1))
    p2 = h1 @ w2.t() + v["fc2.bias"]
    h2 = r(torch.relu(p2))
    z = h2 @ w3.t() + v["fc3.bias"]
    yl = y.reshape(-1).long()
    losses = torch.logsumexp(z, 1) - z.gather(1, yl[:, None])[:, 0]
    dz = r((torch.softmax(z, 1) - F.one_hot(yl, CLASSES).float()) * grad_scale)
    dh2 = r((dz @ w3) * (p2 > 0).float())
    dh1 = r((dh2 @ w2) * (p1 > 0).float())
    # dW1 uses the exact normalised input too: the weight-gradient kernel multiplies the raw
    # u8 pixels (exact in fp16) and applies the normalisation affinely afterwards
    g = torch.cat([(dh1.t() @ xe).reshape(-1), dh1.sum(0), (dh2.t() @ h1).reshape(-1), dh2.sum(0),
                   (dz.t() @ h2).reshape(-1), dz.sum(0)])
    correct = (z.argmax(1) == yl).float().sum()
    return losses.sum(), correct, g


class OptStateCPU:
    """Optimizer state of the CPU trainers beyond ``params`` / ``mom``: AdamW's second moment
    ``v`` and the optimizer step ``opt_step`` (a 1-element tensor, so a regroup broadcasts it
    with the rest), both only where the rule needs them; with ``ema_decay > 0`` the averaged
    parameters ``ema``, their update count ``ema_step`` and the coefficient table ``ema_tab``
    (ops/optim.py ema_table).  This class is the weight EMA's definition on the trainers."""

    def _init_opt(self, kw: dict) -> None:
        self.opt = opt = OptSpec(lr=self.lr, momentum=self.momentum, weight_decay=self.weight_decay, **kw)
        self.mom = torch.zeros_like(self.params) if (self.momentum > 0 or opt.adamw) else None
        self.v = torch.zeros_like(self.params) if opt.adamw else None
        self.opt_step = None if opt.plain else torch.zeros(1, dtype=torch.int32)
        self._grad_norm = None
        self.ema = self.ema_step = self.ema_tab = None
        if opt.emas:  # starts at the initial parameters (flat= included)
            self.ema = self.params.clone()
            self.ema_step = torch.zeros(1, dtype=torch.int32)
            self.ema_tab = torch.from_numpy(opt.ema_table())

    def grad_norm(self) -> float | None:
        """The gradient's global L2 norm at the last step, before clipping (None: clipping off)."""
        return self._grad_norm

    def _opt_update(self, g: torch.Tensor) -> None:
        if self.opt.clips:
            self._grad_norm = clip_grad_(g, self.opt.clip_grad_norm)
        if self.opt_step is None:
            sgd_update(self.params, self.mom, g, self.lr, self.momentum, self.weight_decay)
        else:
            self.opt.update(self.params, self.mom, self.v, g, int(self.opt_step[0]))
            self.opt_step += 1
        if self.ema is not None:  # once per update, on the parameters just written
            t = min(int(self.ema_step[0]), self.ema_tab.numel() - 1)
            ema_update_(self.ema, self.params, self.ema_tab[t])
            self.ema_step += 1

    def ema_flat(self) -> torch.Tensor:
        """A copy of the averaged parameters (``ema_decay > 0``)."""
        if self.ema is None:
            raise ValueError("this trainer keeps no weight EMA (ema_decay=0)")
        return self.ema[:self.n_params].clone()

    def _eval_weights(self, ema: bool) -> torch.Tensor:
        """What ``evaluate(ema=...)`` runs on: the parameters or their average (only read)."""
        if ema and self.ema is None:
            raise ValueError("evaluate(ema=True): this trainer keeps no weight EMA (ema_decay=0)")
        return self.ema if ema else self.params

    def _opt_state_extra(self, d: dict) -> dict:
        if self.opt_step is not None:
            d["opt_step"] = self.opt_step.double().cpu().numpy()
        if self.v is not None:
            d["exp_avg_sq"] = self.v[:self.n_params].double().cpu().numpy()
        if self.ema is not None:
            d["ema"] = self.ema[:self.n_params].double().cpu().numpy()
            d["ema_step"] = self.ema_step.double().cpu().numpy()
        return d

    def _opt_load_state_extra(self, d: dict) -> None:
        if self.opt_step is not None and "opt_step" in d:
            self.opt_step.fill_(int(d["opt_step"][0]))
        if self.v is not None and "exp_avg_sq" in d:
            self.v[:self.n_params].copy_(torch.as_tensor(np.asarray(d["exp_avg_sq"]), dtype=torch.float32))
        if self.ema is not None:
            if "ema" in d and "ema_step" in d:
                self.ema[:self.n_params].copy_(torch.as_tensor(np.asarray(d["ema"]), dtype=torch.float32))
                self.ema_step.fill_(int(d["ema_step"][0]))
            else:  # a checkpoint without one: the average starts over from the weights just loaded
                self.ema.copy_(self.params)
                self.ema_step.zero_()

    def _opt_buffers(self) -> list:
        return [t for t in (self.v, self.opt_step, self.ema, self.ema_step) if t is not None]

    def reset_optimizer_state(self) -> None:
        for t in (self.mom, self.v, self.opt_step):
            if t is not None:
                t.zero_()

    # ---- gradient accumulation: the definition the GPU engines are tested against ----
    accum_steps = 1
    grad = None  # the aggregated gradient of the last step, as the optimizer took it

    def set_accum(self, k) -> None:
        """``k`` micro-batches per optimizer step (one exchange, one clip, one update)."""
        self.accum_steps = check_accum_steps(k)

    @property
    def samples_per_step(self) -> int:
        return self.batch * self.accum_steps

    @property
    def grad_scale(self) -> float:
        """The gradient is a mean over the global batch ``batch * world_size * accum_steps``."""
        return 1.0 / (self.batch * self.world_size * self.accum_steps)

    def _accumulate(self, micro) -> tuple:
        """(loss_sum, correct_sum, g) of one step: ``micro()`` returns them for the micro-batch at
        ``self.cursor``, already scaled by :attr:`grad_scale`; the cursor is bumped between them
        (the step bumps it after the last, with the update), and the micro-gradients are summed in
        fp32 in order, ``((g_0 + g_1) + g_2) + ...``."""
        loss, correct, g = micro()
        for _ in range(1, self.accum_steps):
            self.cursor += 1
            li, ci, gi = micro()
            loss, correct, g = loss + li, correct + ci, g + gi
        return loss, correct, g


@dataclass
class StepStats:
    loss: float
    accuracy: float
    samples: int

    @property
    def n(self) -> int:
        """Samples behind ``loss`` / ``accuracy`` (a training step's: ``accum_steps * batch``)."""
        return self.samples


class CPUTrainer(OptStateCPU):
    """Plain-torch trainer with the same interface as FusedMLPTrainer (CPU workers)."""

    def __init__(self, batch: int, lr: float = 0.05, momentum: float = 0.9,
                 weight_decay: float = 0.0, seed: int = 0, world_size: int = 1,
                 flat: torch.Tensor | None = None, accum_steps: int = 1, **opt):
        self.batch = batch
        self.lr, self.momentum, self.weight_decay = lr, momentum, weight_decay
        self.world_size = world_size
        self.set_accum(accum_steps)
        self.params = (flat if flat is not None else init_params(seed)).clone().float()
        self._init_opt(opt)  # optimizer=, beta1=, beta2=, adam_eps=, lr_schedule=, lr_warmup_steps=, ... (OptSpec)
        self.cursor = 0
        self.x = self.y = None
        self.allreduce = None  # callable(tensor) -> None (sum in place)
        self._last = None
        from ..utils.phases import PhaseProbe

        self.phases = PhaseProbe("cpu")

    n_params = N_PARAMS
    model_name = "mlp-784-256-256-10"

    def layout(self):
        return [[n, list(s), o] for n, s, o, _ in param_layout()]

    def set_world(self, world: int) -> None:
        self.world_size = world

    def refresh_shadows(self) -> None:
        pass

    def load_shard(self, x_u8: torch.Tensor, y_u8: torch.Tensor) -> None:
        assert x_u8.shape[0] >= self.batch
        self.x, self.y = x_u8.reshape(-1, D_IN), y_u8.reshape(-1)
        self.n_batches = self.x.shape[0] // self.batch

    def _micro(self) -> tuple:
        b = self.cursor % self.n_batches
        xs = self.x[b * self.batch:(b + 1) * self.batch]
        ys = self.y[b * self.batch:(b + 1) * self.batch]
        return reference_grads(self.params, xs, ys, self.grad_scale)

    def step(self) -> None:
        loss, correct, g = self._accumulate(self._micro)
        self.phases.mark("compute")
        if self.allreduce is not None:
            self.allreduce(g)
        self.phases.mark("exchange")
        self.grad = g
        self._opt_update(g)
        self.cursor += 1
        self.phases.mark("update")
        self._last = (float(loss), float(correct))

    def probe_step(self):
        """One training step with its phases timed (utils/phases.py; wall clock on the CPU):
        a PendingPhases, ready at once."""
        self.phases.arm()
        self.step()
        pending = self.phases.finish()
        pending.exchange_bytes = 4 * int(self.params.numel()) if self.allreduce is not None else 0
        return pending

    def stats(self) -> StepStats:
        loss, correct = self._last
        n = self.samples_per_step
        return StepStats(loss / n, correct / n, n)

    def evaluate(self, x_u8: torch.Tensor, y_u8: torch.Tensor, ema: bool = False) -> StepStats:
        """Mean loss / accuracy of the parameters (``ema=True``: of their average) over (x, y)."""
        with torch.no_grad():
            logits = MLP(self._eval_weights(ema))(x_u8)
            y = y_u8.reshape(-1).long()
            loss = F.cross_entropy(logits, y, reduction="mean")
            acc = (logits.argmax(1) == y).float().mean()
        return StepStats(float(loss), float(acc), int(y.numel()))

    def evaluate_full(self, x_u8: torch.Tensor, y_u8: torch.Tensor, ema: bool = False, topk: int = 5):
        """The held-out report (ops/evalmetrics.py EvalReport) of the parameters (``ema=True``: of
        their average) over every record of (x, y): the logits of :meth:`evaluate`, the fp32 per-row
        cross-entropy, and the definition itself."""
        from ..ops.evalmetrics import check_records, check_topk, eval_reference

        topk = check_topk(topk, CLASSES)
        w = self._eval_weights(ema)
        y = y_u8.reshape(-1).long()
        check_records(int(y.numel()))
        with torch.no_grad():
            logits = MLP(w)(x_u8)
            rows = F.cross_entropy(logits, torch.where(y < CLASSES, y, 0), reduction="none").float()
        return eval_reference(logits, y, rows, CLASSES, topk)

    def get_flat(self) -> torch.Tensor:
        return self.params.clone()

    def set_flat(self, flat: torch.Tensor) -> None:
        self.params.copy_(flat.to(self.params))

    def state_extra(self) -> dict:
        return self._opt_state_extra({"cursor": np.array([self.cursor], dtype=np.float64)})

    def load_state_extra(self, d: dict) -> None:
        if "cursor" in d:
            self.cursor = int(d["cursor"][0])
        self._opt_load_state_extra(d)

    def buffers(self) -> list:
        return self._opt_buffers()


CPUMLPTrainer = CPUTrainer  # (beside CPUResNetTrainer)


def dh1_scale(grad_scale: float) -> float:
    """Power of two that brings grad_scale-sized dH1 values to O(1) before the rows kernel
    stores them as fp16 for the weight gradient (fp16 would flush them to subnormals)."""
    return 2.0 ** round(-math.log2(grad_scale))


def dw1_coeffs(xa: float, xb: float, scale: float) -> tuple:
    """(a, b) with dW1 = a * slab + b * db1.  The slab holds scale * dH1^T (X + 1024) (the fp16
    GEMM on raw pixels, u -> 1024 + u exactly), and dW1 of the normalised input xa X + xb is
    xa dH1^T X + xb db1 = (xa / scale) slab + (xb - 1024 xa) db1."""
    return xa / scale, xb - 1024.0 * xa


def default_slices(batch: int) -> int:
    """Split-K slices of the weight-gradient GEMM (the kernel's own choice: one workgroup per CU)."""
    from ..ops import _native

    return int(_native.lib().sl_mlp_wgrad_slices(batch, 0))


class FusedMLPTrainer(GraphSlots):
    """MI355X training engine for the MLP: 3 HIP launches per step.

    Buffers are allocated once for a fixed per-GPU batch; the data shard stays
    resident in HBM and a device-side cursor selects the batch, so a step has
    no host work and replays from a hipGraph (:meth:`capture`).
    """

    def __init__(self, batch: int, device="cuda", lr: float = 0.05, momentum: float = 0.9,
                 weight_decay: float = 0.0, seed: int = 0, world_size: int = 1,
                 slices: int | None = None, flat: torch.Tensor | None = None, accum_steps: int = 1, **opt):
        from ..ops import _native

        if batch % BLOCK_ROWS != 0:
            raise ValueError(f"batch must be a multiple of {BLOCK_ROWS}")
        self._n = _native
        _native.lib()  # fail loudly if the HIP library cannot be loaded
        if os.environ.get("SL_MLP_ROWS_BM"):  # force the rows kernel's tile height (64 / 128)
            _native.call("sl_mlp_set_rows_bm", int(os.environ["SL_MLP_ROWS_BM"]))
        dev = torch.device(device)
        self.device = dev
        self.batch = batch
        self.lr, self.momentum, self.weight_decay = lr, momentum, weight_decay
        self.world_size = world_size
        # accum_steps micro-batches per optimizer step: the gradient stays a mean over all of them
        self.accum_steps = check_accum_steps(accum_steps)
        self.grad_scale = 1.0 / (batch * world_size * self.accum_steps)
        s1 = slices or int(os.environ.get("SL_MLP_WG_SLICES", "0") or 0)  # split-K slices (0: library default)
        self.slices = int(_native.lib().sl_mlp_wgrad_slices(batch, s1))
        if self.slices <= 0:
            raise ValueError(f"batch {batch} not supported by the weight-gradient kernel")
        self.xa, self.xb = norm_coeffs()
        n = N_PARAMS
        self.n_pad = (n + 3) // 4 * 4
        self.params = torch.zeros(self.n_pad, dtype=torch.float32, device=dev)
        init = flat if flat is not None else init_params(seed)
        self.params[:n].copy_(init.to(dev))
        # optimizer=, beta1=, beta2=, adam_eps=, lr_schedule=, lr_warmup_steps=, ... (ops.optim.OptSpec)
        self.opt = OptSpec(lr=lr, momentum=momentum, weight_decay=weight_decay, **opt)
        self.mom = torch.zeros_like(self.params) if (momentum > 0 or self.opt.adamw) else None
        # AdamW's second moment (mom is its first); the optimizer step the update kernels read
        # (and its ticket word, mlp_fused.hip opt_end) where the rule depends on the step
        self.v = torch.zeros_like(self.params) if self.opt.adamw else None
        self.opt_step = self.opt_ticket = self.lr_tab = None
        if not self.opt.plain:
            from ..ops.optim import require_kernels

            require_kernels(self.opt, "sl_mlp_opt", "sl_mlp_opt_xgmi")
            self.opt_step = torch.zeros(1, dtype=torch.int32, device=dev)
            self.opt_ticket = torch.zeros(1, dtype=torch.int32, device=dev)
            self._build_lr_table()
        self.clip_partials = self.clip_norm = None
        self._init_clip()
        # the weight EMA (ema_decay > 0): the averaged parameters, the number of EMA updates applied,
        # the ticket word of the launch that advances it and the coefficient table (ops/optim.py
        # ema_table); its shadow set for evaluate(ema=True) is allocated on first use
        self.ema = self.ema_step = self.ema_ticket = self.ema_tab = self._ema_eval = None
        if self.opt.emas:
            from ..ops.optim import EMA_KERNELS, require_kernels

            require_kernels(self.opt, *EMA_KERNELS)
            self.ema = self.params.clone()  # (after flat=)
            self.ema_step = torch.zeros(1, dtype=torch.int32, device=dev)
            self.ema_ticket = torch.zeros(1, dtype=torch.int32, device=dev)
            self._build_ema_table()
        bf = torch.bfloat16
        # W1's shadow is fp16: layer 1 multiplies the exact pixels (fp16 1024 + u) and corrects the
        # offset with the W1 row sums, kept as 64-bit fixed-point partials (mlp_fused.hip, R1_BLK)
        self.w1h = torch.zeros(HIDDEN, D_IN_PAD, dtype=torch.float16, device=dev)
        self.r1p = torch.zeros(HIDDEN * R1_BLK, dtype=torch.int64, device=dev)
        self.w2h = torch.zeros(HIDDEN, HIDDEN, dtype=bf, device=dev)
        self.w2th = torch.zeros(HIDDEN, HIDDEN, dtype=bf, device=dev)
        self.w3h = torch.zeros(16, HIDDEN, dtype=bf, device=dev)
        self.w3th = torch.zeros(HIDDEN, 32, dtype=bf, device=dev)
        # row-major activations for the weight-gradient kernel ([batch][256], dZ [batch][16])
        self.h1t = torch.empty(batch, HIDDEN, dtype=bf, device=dev)
        self.dh1t = torch.empty(batch, HIDDEN, dtype=bf, device=dev)
        self.dh2t = torch.empty(batch, HIDDEN, dtype=bf, device=dev)
        # per-64-row partials of [dW3 | db3] from the rows kernel (H2 / dZ never reach HBM)
        self.w3p = torch.empty(batch // 64, W3P_LD, dtype=torch.float32, device=dev)
        self.loss = torch.zeros(batch, dtype=torch.float32, device=dev)
        self.correct = torch.zeros(batch, dtype=torch.float32, device=dev)
        # per-slice stride of the weight-gradient slab (the kernel library's layout: tiled in the
        # wgrad kernel's register order, larger than the parameter count)
        lib = _native.lib()
        # (older kernel builds, kept for A/B runs, have no tiled layout and no stride query)
        self.slab_stride = int(lib.sl_mlp_slab_stride()) if hasattr(lib, "sl_mlp_slab_stride") else self.n_pad
        self.slab = torch.empty(self.slices, self.slab_stride, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(self.n_pad, dtype=torch.float32, device=dev)
        # gradient accumulation's partial sums (gradient, per-sample loss and correct): None at accum_steps 1
        self.acc = self.loss_acc = self.correct_acc = None
        self._alloc_accum()
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.allreduce = None  # callable(grad_tensor) -> None, sums in place (RCCL)
        self.xgmi = None       # parallel.xgmi.XgmiExchange: all-reduce fused into the update (no RCCL)
        self.x = self.y = None
        self.xt = None         # the shard in 64 x 64-byte bricks: what the training launches read
        self.n_batches = 1
        self.graph = None
        from ..utils.phases import PhaseProbe

        self.phases = PhaseProbe(dev)
        self.refresh_shadows()
        # torch loads its reduction kernel's code object on first use (~27 ms): take that here,
        # at construction, not in the first logged chunk of a training worker (profiles/r04_runtime)
        self.stats()

    n_params = N_PARAMS
    model_name = "mlp-784-256-256-10"

    def layout(self):
        return [[n, list(s), o] for n, s, o, _ in param_layout()]

    def set_world(self, world: int) -> None:
        """Gradient scale follows the group size (mean over the global batch)."""
        self.world_size = world
        self.grad_scale = 1.0 / (self.batch * world * self.accum_steps)
        self.graph = None

    def _alloc_accum(self) -> None:
        if self.accum_steps == 1:
            self.acc = self.loss_acc = self.correct_acc = None
        elif self.acc is None:
            from ..ops.optim import ACCUM_KERNELS, require_kernels

            require_kernels(self.opt, *ACCUM_KERNELS, "sl_cursor_bump")
            self.acc = torch.zeros_like(self.grad)
            self.loss_acc, self.correct_acc = torch.zeros_like(self.loss), torch.zeros_like(self.correct)

    def set_accum(self, k: int) -> None:
        """``k`` micro-batches per optimizer step: each runs rows / wgrad / reduce on its own batch
        (the cursor moves after each), the reduced gradients are summed in fp32 in order, and the
        sum takes the exchange hook, the clip and one update.  The gradient scale follows (a mean
        over ``k * batch * world``); the launches are rebuilt and the captured graphs dropped.
        Not with the xGMI exchange, which reduces the slab straight into its slot."""
        k = check_accum_steps(k)
        if k > 1 and self.xgmi is not None:
            raise ValueError("gradient accumulation is not available with the xGMI exchange "
                             "(keep the process group's all-reduce)")
        self.accum_steps = k
        self._alloc_accum()
        self.set_world(self.world_size)
        self.graph_unrolled = None

    @property
    def samples_per_step(self) -> int:
        return self.batch * self.accum_steps

    # ---- data ----
    def load_shard(self, x_u8: torch.Tensor, y_u8: torch.Tensor) -> None:
        """Make a device-resident shard current ([N,784] u8 images, [N] u8 labels)."""
        x = x_u8.reshape(-1, D_IN)
        if x.shape[0] < self.batch:
            raise ValueError("shard smaller than one batch")
        self.x = x.to(self.device, non_blocking=True).contiguous()
        self.y = y_u8.reshape(-1).to(self.device, non_blocking=True).to(torch.uint8).contiguous()
        self.n_batches = self.x.shape[0] // self.batch
        # The training launches re-read the shard every step: laid out once in 4 KB bricks
        # (xt[rows / 64][13][64][64], mlp_fused.hip XT_BRICK) every X access of theirs is whole
        # aligned cache lines.  SL_MLP_XTILE=0 keeps them on the row-major shard (A/B, tests);
        # older kernel builds, kept for A/B runs, have no tiled entry points.
        self.xt = None
        lib = self._n.lib()
        if os.environ.get("SL_MLP_XTILE", "1") != "0" and hasattr(lib, "sl_mlp_x_tile"):
            rows = self.n_batches * self.batch
            self.xt = torch.empty(int(lib.sl_mlp_x_tile_bytes(rows)), dtype=torch.uint8, device=self.device)
            self._n.call("sl_mlp_x_tile", self._n.ptr(self.x), self._n.ptr(self.xt), rows, self._n.stream_ptr())
        self.graph = None

    # ---- kernels ----
    def refresh_shadows(self) -> None:
        n = self._n
        n.call("sl_mlp_sgd", n.ptr(self.params), None, None, 0, 0, None, None, 0.0, 0.0, 0.0, self.xa, self.xb, 0,
               n.ptr(self.w1h), n.ptr(self.w2h), n.ptr(self.w2th), n.ptr(self.w3h), n.ptr(self.w3th),
               None, n.ptr(self.r1p), n.stream_ptr())

    @property
    def dh1_scale(self) -> float:
        return dh1_scale(self.grad_scale)

    @property
    def dw1_coeffs(self) -> tuple:
        return dw1_coeffs(self.xa, self.xb, self.dh1_scale)

    def _build_lr_table(self) -> None:
        tab = self.opt.lr_table()
        self.lr_tab = torch.from_numpy(tab).to(self.device) if tab is not None else None

    def _build_ema_table(self) -> None:
        self.ema_tab = torch.from_numpy(self.opt.ema_table()).to(self.device)

    def _init_clip(self) -> None:
        """Gradient clipping's scratch (the workgroups' fp64 partial sums) and the norm it reports."""
        if self.opt.clips and self.clip_norm is None:
            from ..ops.optim import CLIP_KERNELS, clip_buffers, require_kernels

            require_kernels(self.opt, *CLIP_KERNELS)
            self.clip_partials, self.clip_norm = clip_buffers(N_PARAMS, self.device)

    def set_optimizer(self, **kw) -> None:
        """Change optimizer hyper-parameters (OptSpec fields; ``clip_grad_norm`` under any rule,
        the others of a step-counter rule): the launches are rebuilt and the captured graphs
        dropped, as a new ``lr`` does.  The rule itself (which state exists) is fixed at
        construction."""
        import dataclasses

        if self.opt.plain:  # a plain rule's lr / momentum / weight_decay live in the attributes
            kw = {"lr": self.lr, "momentum": self.momentum, "weight_decay": self.weight_decay, **kw}
        new = dataclasses.replace(self.opt, **kw)
        if (new.adamw, new.plain) != (self.opt.adamw, self.opt.plain):
            raise ValueError("the optimizer rule is fixed at construction (build a new trainer)")
        if new.emas != self.opt.emas:
            raise ValueError("the weight EMA is switched on or off at construction (build a new trainer)")
        if new.clips and self.xgmi is not None:
            raise ValueError("gradient clipping is not available with the xGMI exchange")
        self.opt = new
        self.lr, self.momentum, self.weight_decay = new.lr, new.momentum, new.weight_decay
        if not new.plain:
            self._build_lr_table()
        if new.emas:
            self._build_ema_table()
        self._init_clip()
        self.graph = None
        self._lkey = None

    def _launches(self):
        """Cached launches for the current buffers/hyper-parameters (rebuilt on change)."""
        hp = (self.lr, self.momentum, self.weight_decay)
        if not self.opt.plain and hp != (self.opt.lr, self.opt.momentum, self.opt.weight_decay):
            self.set_optimizer(lr=hp[0], momentum=hp[1], weight_decay=hp[2])  # an attribute was assigned
        key = (self.x.data_ptr() if self.x is not None else 0, self.xt.data_ptr() if self.xt is not None else 0,
               self.n_batches, self.grad_scale, self.lr,
               self.momentum, self.weight_decay, id(self.xgmi), bool(self.xgmi and self.xgmi.two_shot),
               self.xgmi.inline_sync if self.xgmi is not None else None, None if self.opt.plain else self.opt,
               self.opt.clip_grad_norm, self.accum_steps,
               (self.opt.ema_decay, self.opt.ema_warmup) if self.opt.emas else None)
        if getattr(self, "_lkey", None) == key:
            return self._lc
        n, p = self._n, self._n.ptr
        ws = (p(self.w1h), p(self.w2h), p(self.w2th), p(self.w3h), p(self.w3th))
        # X from the tiled shard where there is one (load_shard): the same launches through their
        # tiled entry points
        xsrc, sfx = (self.xt, "_xt") if self.xt is not None else (self.x, "")
        lc = {
            "rows": n.Launch("sl_mlp_rows", p(xsrc), p(self.y), p(self.cursor), self.n_batches, self.batch,
                             p(self.w1h), p(self.w2h), p(self.w3h), p(self.w2th), p(self.w3th),
                             p(self.params), self.xa, self.xb, self.grad_scale, self.dh1_scale,
                             p(self.h1t), p(self.w3p), p(self.dh2t), p(self.dh1t),
                             p(self.loss), p(self.correct), None, 1, p(self.r1p),
                             # xGMI inline synchronisation: this launch advances the exchange's step id
                             self.xgmi.ctl.data_ptr() if self.xgmi is not None and self.xgmi.inline_sync else None,
                             entry="sl_mlp_rows" + sfx),
            "wgrad": n.Launch("sl_mlp_wgrad", self.batch, p(xsrc), p(self.cursor), self.n_batches,
                              p(self.h1t), p(self.dh2t), p(self.dh1t), p(self.w3p), self.w3p.shape[0], p(self.slab),
                              self.slices, self.slab_stride, entry="sl_mlp_wgrad" + sfx),
        }
        for name, (mode, from_grad, grad_out, bump) in {"sgd": (2, False, False, True),
                                                        "reduce": (1, False, True, False),
                                                        "update": (2, True, False, True)}.items():
            if mode == 2 and not self.opt.plain:  # the update under a step-counter rule (reduce: rule-independent)
                lc[name] = n.Launch("sl_mlp_opt", self.opt.rule, p(self.params), p(self.mom), p(self.v),
                                    None if from_grad else p(self.slab), self.slices, self.slab_stride,
                                    p(self.grad) if from_grad else None, self.lr, self.momentum, self.weight_decay,
                                    *self.dw1_coeffs, *ws, p(self.cursor), p(self.r1p), *self._opt_args())
                continue
            lc[name] = n.Launch("sl_mlp_sgd", p(self.params), p(self.mom),
                                None if from_grad else p(self.slab), self.slices, self.slab_stride,
                                p(self.grad) if from_grad else None, p(self.grad) if grad_out else None,
                                self.lr, self.momentum, self.weight_decay, *self.dw1_coeffs, mode, *ws,
                                p(self.cursor) if bump else None, p(self.r1p))
        if self.opt.clips:  # between the reduce and the update launches, on the real parameters only
            lc["clip"] = n.Launch("sl_clip_grad_norm", p(self.grad), N_PARAMS, self.opt.clip_grad_norm,
                                  p(self.clip_partials), self.clip_partials.numel(), p(self.clip_norm))
        if self.accum_steps > 1:
            # the sums of an accumulated step: store after micro-batch 0, add after 1 .. K-2, and the
            # fold of the partial sums into grad / loss / correct after the last; the earlier
            # micro-batches' cursor bump (the update launch bumps it after the last)
            pairs = ((self.acc, self.grad, N_PARAMS), (self.loss_acc, self.loss, self.batch),
                     (self.correct_acc, self.correct, self.batch))
            for name, add in (("acc_store", 0), ("acc_add", 1)):
                lc[name] = [n.Launch("sl_accum_flat", p(a), p(t), cnt, add) for a, t, cnt in pairs]
            lc["acc_fold"] = [n.Launch("sl_accum_flat", p(t), p(a), cnt, 1) for a, t, cnt in pairs]
            lc["bump"] = n.Launch("sl_cursor_bump", p(self.cursor))
        if self.opt.emas:  # after the update launch of every step path; advances ema_step itself
            lc["ema"] = n.Launch("sl_ema_flat", p(self.ema), p(self.params), N_PARAMS, p(self.ema_step),
                                 p(self.ema_ticket), p(self.ema_tab), self.ema_tab.numel())
        if self.xgmi is not None:
            xg = self.xgmi
            # inline synchronisation: the reduce publishes the step, the update waits per workgroup
            lc["xreduce"] = n.Launch("sl_mlp_reduce_xgmi", p(self.slab), self.slices, self.slab_stride, *self.dw1_coeffs,
                                     xg.slot_ptr(0), xg.slot_ptr(1), *xg.args(), xg.inline_sync)
            lc["xbarrier"] = [n.Launch(fn, *xg.args(), *extra) for fn, extra in xg.exchange_launches(self.n_pad)]
            if self.opt.plain:
                lc["xupdate"] = n.Launch("sl_mlp_sgd_xgmi", p(self.params), p(self.mom), self.lr, self.momentum,
                                         self.weight_decay, *ws, p(self.cursor), *xg.args(), p(self.r1p),
                                         xg.inline_sync)
            else:
                lc["xupdate"] = n.Launch("sl_mlp_opt_xgmi", self.opt.rule, p(self.params), p(self.mom), p(self.v),
                                         self.lr, self.momentum, self.weight_decay, *ws, p(self.cursor), *xg.args(),
                                         p(self.r1p), xg.inline_sync, *self._opt_args())
        self._lc, self._lkey = lc, key
        return lc

    def _opt_args(self) -> tuple:
        """Trailing arguments of sl_mlp_opt / sl_mlp_opt_xgmi: step, ticket, lr table, Adam scalars."""
        p = self._n.ptr
        return (p(self.opt_step), p(self.opt_ticket), p(self.lr_tab),
                self.lr_tab.numel() if self.lr_tab is not None else 0, *self.opt.adam_scalars())

    def _rows(self, train: bool = True):
        if train:
            return self._launches()["rows"]()
        n = self._n
        n.call("sl_mlp_rows", n.ptr(self.x), n.ptr(self.y), n.ptr(self.cursor), self.n_batches, self.batch,
               n.ptr(self.w1h), n.ptr(self.w2h), n.ptr(self.w3h), n.ptr(self.w2th), n.ptr(self.w3th),
               n.ptr(self.params), self.xa, self.xb, self.grad_scale, self.dh1_scale,
               n.ptr(self.h1t), n.ptr(self.w3p), n.ptr(self.dh2t), n.ptr(self.dh1t),
               n.ptr(self.loss), n.ptr(self.correct), None, 0, n.ptr(self.r1p), None, n.stream_ptr())

    def _wgrad(self):
        self._launches()["wgrad"]()

    def _sgd(self, mode: int, from_grad: bool, grad_out: bool, bump: bool = True):
        name = {(2, False, False, True): "sgd", (1, False, True, False): "reduce",
                (2, True, False, True): "update"}[(mode, from_grad, grad_out, bump)]
        self._launches()[name]()

    def compute_grads(self) -> torch.Tensor:
        """Forward + backward only; returns the reduced (local) gradient (not with an xGMI
        exchange enabled: its rows launch advances the exchange's step id)."""
        self._rows(True)
        self._wgrad()
        self._sgd(1, from_grad=False, grad_out=True, bump=False)
        return self.grad[:N_PARAMS]

    def step(self) -> None:
        if self.graph is not None:
            self.graph.replay()
            return
        self._step_eager()

    def steps(self, n: int) -> None:
        """Run ``n`` full training steps.  With a multi-step graph captured
        (``capture(unroll=k)``) they replay k at a time: the ~8 us gap that every
        graph launch leaves between the previous step's SGD and the next rows
        kernel is paid once per k steps (every step still runs all three kernels
        on its own batch; the device cursor advances inside the graph)."""
        g, k = getattr(self, "graph_unrolled", None), getattr(self, "unroll", 1)
        if self.graph is not None and g is not None and k > 1:  # self.graph=None invalidates both
            while n >= k:
                g.replay()
                n -= k
        for _ in range(n):
            self.step()

    def enable_xgmi(self, exchange) -> None:
        """Aggregate gradients through an :class:`~serverless_learn_amd.parallel.xgmi.XgmiExchange`
        (the slab reduction lands in this rank's exchange slot; the update kernel sums every
        rank's slot over xGMI and applies SGD).  ``None`` switches back.  Not with gradient
        clipping: the summed gradient never exists before that update."""
        if exchange is not None and self.opt.clips:
            raise ValueError("gradient clipping is not available with the xGMI exchange "
                             "(keep the process-group all-reduce)")
        if exchange is not None and self.accum_steps > 1:
            raise ValueError("gradient accumulation is not available with the xGMI exchange "
                             "(keep the process-group all-reduce)")
        if exchange is not None and exchange.payload_floats < self.n_pad:
            raise ValueError("exchange slot smaller than the parameter vector")
        self.xgmi = exchange
        self.graph = None
        self._lkey = None

    def enable_clock_probe(self, cap: int = 16 * 2048) -> None:
        """Diagnostics (bench.py SL_CLOCK_PROBE=1): a 16-workgroup kernel stamps (XCC id,
        shader clock, 100 MHz wall clock) at the start of every step, inside the captured
        graphs too (csrc/kernels/diag.hip)."""
        self.probe_buf = torch.zeros(3 * cap, dtype=torch.int64, device=self.device)
        self.probe_cnt = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.probe = self._n.Launch("sl_clock_probe", self._n.ptr(self.probe_buf), self._n.ptr(self.probe_cnt), cap)
        self.graph = None

    def clock_probe_steps(self) -> list:
        """Per probed step boundary: (wall time in us of the 100 MHz clock, {xcc: shader ticks})."""
        n = min(int(self.probe_cnt.item()), self.probe_buf.numel() // 3)
        rec = self.probe_buf[:3 * n].view(n, 3).cpu().tolist()
        out = []
        for i in range(0, n - n % 16, 16):  # one launch = 16 consecutive records
            grp = rec[i:i + 16]
            wall = min(r[2] for r in grp)
            ticks = {}
            for x, t, w in grp:
                ticks.setdefault(x, (t, w))
            out.append((wall, ticks))
        return out

    def _step_eager(self) -> None:
        if getattr(self, "probe", None) is not None:
            self.probe()
        ph = self.phases
        if self.accum_steps > 1:
            return self._step_accum()
        self._rows(True)
        self._wgrad()
        ph.mark("compute")
        if self.xgmi is not None:
            lc = self._launches()
            lc["xreduce"]()
            for launch in lc["xbarrier"]:
                launch()
            ph.mark("exchange")  # slab reduction into the exchange slot + the step barrier(s)
            lc["xupdate"]()      # (the peers' slots are summed inside the update kernel)
        elif self.allreduce is None and not self.opt.clips:
            self._sgd(2, from_grad=False, grad_out=False)
        else:
            self._sgd(1, from_grad=False, grad_out=True, bump=False)
            if self.allreduce is not None:
                self.allreduce(self.grad)
                ph.mark("exchange")
            if self.opt.clips:  # the whole norm before any weight moves: the fused slab update cannot clip
                self._launches()["clip"]()
            self._sgd(2, from_grad=True, grad_out=False)
        if self.ema is not None:  # local, so also behind the xGMI update
            self._launches()["ema"]()
        ph.mark("update")

    def _step_accum(self) -> None:
        """One step of ``accum_steps`` micro-batches: grad = ((g_0 + g_1) + ...) + g_last, then the
        reduce -> hook -> clip -> update path of a clipping step (no fused slab update)."""
        lc, ph, last = self._launches(), self.phases, self.accum_steps - 1
        for i in range(last + 1):
            lc["rows"]()
            lc["wgrad"]()
            lc["reduce"]()
            for launch in lc["acc_fold" if i == last else "acc_add" if i else "acc_store"]:
                launch()
            if i < last:
                lc["bump"]()
        ph.mark("compute")
        if self.allreduce is not None:
            self.allreduce(self.grad)
            ph.mark("exchange")
        if self.opt.clips:
            lc["clip"]()
        lc["update"]()
        if self.ema is not None:
            lc["ema"]()
        ph.mark("update")

    def grad_norm(self) -> float | None:
        """The aggregated gradient's global L2 norm at the last step, before clipping (one float
        read from the device); None with clipping off."""
        return float(self.clip_norm[0]) if self.opt.clips else None

    def probe_step(self):
        """One eager training step with its phase boundaries recorded (utils/phases.py): returns
        a PendingPhases (resolved by the caller once the device has finished the step) carrying
        the gradient payload aggregated per step (fp32 bytes, 0 at world 1)."""
        self.phases.arm()
        self._step_eager()
        pending = self.phases.finish()
        pending.exchange_bytes = 4 * N_PARAMS if (self.allreduce is not None or self.xgmi is not None) else 0
        return pending

    def drop_graphs(self) -> None:
        """Release every captured step graph after the device has finished with them.  A
        graph may hold a communicator's kernels: the runtime calls this before it re-forms or
        tears down the group, so no replay is in flight when the old
        communicator goes away and the k-step graph is not left alive holding it."""
        if self.graph is not None or self.retired_graphs:  # steps() ignores graph_unrolled once graph is None
            torch.cuda.synchronize(self.device)
        self.graph = None
        self.graph_unrolled = None
        self.reap_graphs(sync=False)

    def capture(self, warmup: int = 2, unroll: int = 1) -> None:
        """Capture one step into a hipGraph (kernels only, or kernels + RCCL);
        ``unroll > 1`` also captures a k-step graph used by :meth:`steps`.  Graphs replaced
        since the last capture are freed first, after a device sync (utils/graphs.py)."""
        self.reap_graphs()
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._step_eager()
        torch.cuda.current_stream(self.device).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step_eager()
        self.graph = g
        self.graph_unrolled, self.unroll = None, max(1, int(unroll))
        if self.unroll > 1:
            gk = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gk):
                for _ in range(self.unroll):
                    self._step_eager()
            self.graph_unrolled = gk

    # ---- eval / state ----
    def w1_out_of_range(self) -> bool:
        """True when a W1 weight no longer fits the fp16 shadow layer 1 runs on (|w| >= 65488):
        the SGD kernel saturates that shadow entry and flags its row sum (mlp_fused.hip h_fix)."""
        return int(self.r1p.max()) >= R1_OVF_MIN

    def stats(self) -> StepStats:
        loss = float(self.loss.sum())
        acc = float(self.correct.sum())
        if self.w1_out_of_range():
            loss = float("nan")  # visible: never a number from a saturated layer 1
        n = self.samples_per_step  # (an accumulated step leaves the sums over its micro-batches in loss / correct)
        return StepStats(loss / n, acc / n, n)

    def ema_flat(self) -> torch.Tensor:
        """A copy of the averaged parameters (``ema_decay > 0``)."""
        if self.ema is None:
            raise ValueError("this trainer keeps no weight EMA (ema_decay=0)")
        return self.ema[:N_PARAMS].clone()

    def _eval_set(self, ema: bool) -> dict:
        """The weights an evaluation launch reads: the training set, or with ``ema`` a second set
        of shadows (allocated on first use) rebuilt from the averaged parameters by the launch that
        ``refresh_shadows`` uses -- what a second trainer holds after ``set_flat(ema_flat())``.  No
        training tensor is written or moved, so a captured graph stays valid."""
        names = ("w1h", "w2h", "w2th", "w3h", "w3th", "r1p")
        if not ema:
            return dict({k: getattr(self, k) for k in names}, params=self.params)
        if self.ema is None:
            raise ValueError("ema=True: this trainer keeps no weight EMA (ema_decay=0)")
        if self._ema_eval is None:
            self._ema_eval = {k: torch.zeros_like(getattr(self, k)) for k in names}
        s, n = self._ema_eval, self._n
        n.call("sl_mlp_sgd", n.ptr(self.ema), None, None, 0, 0, None, None, 0.0, 0.0, 0.0, self.xa, self.xb, 0,
               n.ptr(s["w1h"]), n.ptr(s["w2h"]), n.ptr(s["w2th"]), n.ptr(s["w3h"]), n.ptr(s["w3th"]),
               None, n.ptr(s["r1p"]), n.stream_ptr())
        return dict(s, params=self.ema)

    def evaluate(self, x_u8: torch.Tensor, y_u8: torch.Tensor, ema: bool = False) -> StepStats:
        """Mean loss / accuracy over the whole 64-row blocks of (x, y); ``ema=True``: of the
        averaged parameters, the training state untouched (between steps)."""
        n = self._n
        s = self._eval_set(ema)
        x = x_u8.reshape(-1, D_IN).to(self.device).contiguous()
        y = y_u8.reshape(-1).to(self.device).to(torch.uint8).contiguous()
        rows = x.shape[0] // BLOCK_ROWS * BLOCK_ROWS
        loss = torch.zeros(rows, device=self.device)
        corr = torch.zeros(rows, device=self.device)
        n.call("sl_mlp_rows", n.ptr(x), n.ptr(y), None, 1, rows,
               n.ptr(s["w1h"]), n.ptr(s["w2h"]), n.ptr(s["w3h"]), n.ptr(s["w2th"]), n.ptr(s["w3th"]),
               n.ptr(s["params"]), self.xa, self.xb, 1.0, 1.0, None, None, None, None,
               n.ptr(loss), n.ptr(corr), None, 0, n.ptr(s["r1p"]), None, n.stream_ptr())
        lv = float("nan") if int(s["r1p"].max()) >= R1_OVF_MIN else float(loss.mean())
        return StepStats(lv, float(corr.mean()), rows)

    def logits(self, x_u8: torch.Tensor, ema: bool = False) -> torch.Tensor:
        n = self._n
        s = self._eval_set(ema)
        x = x_u8.reshape(-1, D_IN).to(self.device).contiguous()
        rows = x.shape[0]
        if rows % BLOCK_ROWS:
            raise ValueError(f"rows must be a multiple of {BLOCK_ROWS}")
        out = torch.empty(rows, CLASSES, device=self.device)
        n.call("sl_mlp_rows", n.ptr(x), None, None, 1, rows,
               n.ptr(s["w1h"]), n.ptr(s["w2h"]), n.ptr(s["w3h"]), n.ptr(s["w2th"]), n.ptr(s["w3th"]),
               n.ptr(s["params"]), self.xa, self.xb, 1.0, 1.0, None, None, None, None,
               None, None, n.ptr(out), 0, n.ptr(s["r1p"]), None, n.stream_ptr())
        if int(s["r1p"].max()) >= R1_OVF_MIN:
            out.fill_(float("nan"))
        return out

    def evaluate_full(self, x_u8: torch.Tensor, y_u8: torch.Tensor, ema: bool = False, topk: int = 5):
        """The held-out report (ops/evalmetrics.py EvalReport) over every record of (x, y), padded
        with zero rows to whole 64-row blocks: one evaluation-form rows launch writes the per-row loss
        and the logits, one ``sl_eval_accum`` launch over all rows with ``n_valid = N`` counts them on
        the device, and the 264-word block is read once.  ``ema=True``: of the averaged parameters;
        the training state is untouched (between steps).  A W1 weight beyond fp16 (``stats``' rule)
        makes every row bad and the loss NaN."""
        from ..ops import evalmetrics as E

        n = self._n
        topk = E.check_topk(topk, CLASSES)
        y = y_u8.reshape(-1)
        N = E.check_records(int(y.numel()))
        x = x_u8.reshape(N, D_IN)
        s = self._eval_set(ema)
        rows = (N + BLOCK_ROWS - 1) // BLOCK_ROWS * BLOCK_ROWS
        xp = torch.zeros(rows, D_IN, dtype=torch.uint8, device=self.device)
        yp = torch.zeros(rows, dtype=torch.uint8, device=self.device)
        xp[:N].copy_(x)
        yp[:N].copy_(y)
        loss = torch.empty(rows, device=self.device)
        out = torch.empty(rows, CLASSES, device=self.device)
        acc = E.new_acc(self.device)
        n.call("sl_mlp_rows", n.ptr(xp), n.ptr(yp), None, 1, rows,
               n.ptr(s["w1h"]), n.ptr(s["w2h"]), n.ptr(s["w3h"]), n.ptr(s["w2th"]), n.ptr(s["w3th"]),
               n.ptr(s["params"]), self.xa, self.xb, 1.0, 1.0, None, None, None, None,
               n.ptr(loss), None, n.ptr(out), 0, n.ptr(s["r1p"]), None, n.stream_ptr())
        E.eval_accum(out, yp, loss, N, CLASSES, topk, acc)
        rep = E.report_from_acc(acc, CLASSES, topk)
        return rep.all_bad() if int(s["r1p"].max()) >= R1_OVF_MIN else rep

    def get_flat(self) -> torch.Tensor:
        return self.params[:N_PARAMS].clone()

    def set_flat(self, flat: torch.Tensor) -> None:
        self.params[:N_PARAMS].copy_(flat.to(self.params))
        self.refresh_shadows()

    # ---- exact-resume state beyond the flat vectors (ckpt format v2) ----
    def state_extra(self) -> dict:
        """The device batch cursor: a resumed run continues with the batch the saved run
        would have taken next, so save-at-k + resume + m steps equals k + m steps."""
        d = {"cursor": self.cursor.double().cpu().numpy()}
        if self.opt_step is not None:  # the optimizer step and AdamW's second moment (the first
            d["opt_step"] = self.opt_step.double().cpu().numpy()  # travels as the momentum section)
        if self.v is not None:
            d["exp_avg_sq"] = self.v[:N_PARAMS].double().cpu().numpy()
        if self.ema is not None:  # the averaged parameters and the number of EMA updates behind them
            d["ema"] = self.ema[:N_PARAMS].double().cpu().numpy()
            d["ema_step"] = self.ema_step.double().cpu().numpy()
        return d

    def load_state_extra(self, d: dict) -> None:
        if "cursor" in d:
            self.cursor.fill_(int(d["cursor"][0]))
        if self.opt_step is not None:
            if "opt_step" in d:
                self.opt_step.fill_(int(d["opt_step"][0]))
            self.opt_ticket.zero_()
        if self.v is not None and "exp_avg_sq" in d:
            self.v[:N_PARAMS].copy_(torch.as_tensor(np.asarray(d["exp_avg_sq"]), dtype=torch.float32))
        if self.ema is not None:
            if "ema" in d and "ema_step" in d:
                self.ema[:N_PARAMS].copy_(torch.as_tensor(np.asarray(d["ema"]), dtype=torch.float32))
                self.ema_step.fill_(int(d["ema_step"][0]))
            else:  # a checkpoint without one: the average starts over from the weights just loaded
                self.ema.copy_(self.params)
                self.ema_step.zero_()
            self.ema_ticket.zero_()

    def buffers(self) -> list:
        """Optimizer state beyond params / mom (and the weight EMA), broadcast with them after a
        regroup."""
        return [t for t in (self.v, self.opt_step, self.ema, self.ema_step) if t is not None]

    def reset_optimizer_state(self) -> None:
        for t in (self.mom, self.v, self.opt_step, self.opt_ticket):
            if t is not None:
                t.zero_()
