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

import torch
import torch.nn as nn
import torch.nn.functional as F

# (the rules' semantics live there)
from ..ops.optim import (ACCUM_KERNELS, OptSpec, adamw_update, check_accum_steps, clip_grad_,  # noqa: F401
                         ema_update_, lr_at, sgd_update)
from ..utils.graphs import GraphedStep
from .trainer_state import CPUTrainerBase, StepStats, TrainerState  # noqa: F401  (StepStats: imported from here)

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


class CPUTrainer(CPUTrainerBase):
    """Plain-torch trainer with the same interface as FusedMLPTrainer (CPU workers)."""

    def __init__(self, batch: int, lr: float = 0.05, momentum: float = 0.9,
                 weight_decay: float = 0.0, seed: int = 0, world_size: int = 1,
                 flat: torch.Tensor | None = None, accum_steps: int = 1, **opt):
        self._init_cpu(flat if flat is not None else init_params(seed), batch, lr, momentum, weight_decay,
                       world_size, accum_steps, opt)

    n_params = N_PARAMS
    model_name = "mlp-784-256-256-10"

    def layout(self):
        return [[n, list(s), o] for n, s, o, _ in param_layout()]

    def load_shard(self, x_u8: torch.Tensor, y_u8: torch.Tensor) -> None:
        assert x_u8.shape[0] >= self.batch
        self.x, self.y = x_u8.reshape(-1, D_IN), y_u8.reshape(-1)
        self.n_batches = self.x.shape[0] // self.batch

    def _micro(self) -> tuple:
        b = self.cursor % self.n_batches
        xs = self.x[b * self.batch:(b + 1) * self.batch]
        ys = self.y[b * self.batch:(b + 1) * self.batch]
        return reference_grads(self.params, xs, ys, self.grad_scale)

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


class FusedMLPTrainer(GraphedStep, TrainerState):
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
        self._init_state(batch, lr, momentum, weight_decay, world_size, accum_steps, opt)
        self._ema_eval = None  # the EMA's shadow set for evaluate(ema=True), allocated on first use
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
        self._alloc_accum()
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.allreduce = None  # callable(grad_tensor) -> None, sums in place (RCCL)
        self.xgmi = None       # parallel.xgmi.XgmiExchange: all-reduce fused into the update (no RCCL)
        self.x = self.y = None
        self.xt = None         # the shard in 64 x 64-byte bricks: what the training launches read
        self.n_batches = 1
        from ..utils.phases import PhaseProbe

        self.phases = PhaseProbe(dev)
        self.refresh_shadows()
        # torch loads its reduction kernel's code object on first use (~27 ms): take that here,
        # at construction, not in the first logged chunk of a training worker (profiles/r04_runtime)
        self.stats()

    n_params = N_PARAMS
    model_name = "mlp-784-256-256-10"

    tickets = ("opt_ticket", "ema_ticket")  # (mlp_fused.hip opt_end; elementwise.hip sl_ema_flat)
    opt_kernels = ("sl_mlp_opt", "sl_mlp_opt_xgmi")
    group_kernels = ("sl_mlp_opt_groups", "sl_mlp_opt_xgmi_groups")
    accum_kernels = (*ACCUM_KERNELS, "sl_cursor_bump")

    def layout(self):
        return [[n, list(s), o] for n, s, o, _ in param_layout()]

    def set_accum(self, k: int) -> None:
        """:meth:`TrainerState.set_accum`: each micro-batch runs rows / wgrad / reduce, and the sum
        takes the exchange hook, the clip and one update; the launches are rebuilt and the captured
        graphs dropped.  Not with the xGMI exchange, which reduces the slab straight into its slot."""
        if check_accum_steps(k) > 1 and self.xgmi is not None:
            raise ValueError("gradient accumulation is not available with the xGMI exchange "
                             "(keep the process group's all-reduce)")
        super().set_accum(k)
        self.graph_unrolled = None

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
    SHADOWS = ("w1h", "w2h", "w2th", "w3h", "w3th", "r1p")

    def _build_shadows(self, flat: torch.Tensor, s: dict) -> None:
        """The shadow set ``s`` (:attr:`SHADOWS` by name) of the flat vector ``flat``: the update
        launch with nothing to apply."""
        n = self._n
        n.call("sl_mlp_sgd", n.ptr(flat), None, None, 0, 0, None, None, 0.0, 0.0, 0.0, self.xa, self.xb, 0,
               n.ptr(s["w1h"]), n.ptr(s["w2h"]), n.ptr(s["w2th"]), n.ptr(s["w3h"]), n.ptr(s["w3th"]),
               None, n.ptr(s["r1p"]), n.stream_ptr())

    def refresh_shadows(self) -> None:
        self._build_shadows(self.params, self._eval_set(False))

    @property
    def dh1_scale(self) -> float:
        return dh1_scale(self.grad_scale)

    @property
    def dw1_coeffs(self) -> tuple:
        return dw1_coeffs(self.xa, self.xb, self.dh1_scale)

    def set_optimizer(self, **kw) -> None:
        """Change optimizer hyper-parameters (OptSpec fields; ``clip_grad_norm`` under any rule,
        the others of a step-counter rule): the launches are rebuilt and the captured graphs
        dropped, as a new ``lr`` does.  The rule itself (which state exists) is fixed at
        construction, and so is whether the decay groups are on (their values may change)."""
        import dataclasses

        if self.opt.plain:  # a plain rule's lr / momentum / weight_decay live in the attributes
            kw = {"lr": self.lr, "momentum": self.momentum, "weight_decay": self.weight_decay, **kw}
        new = dataclasses.replace(self.opt, **kw)
        if new.grouped != self.opt.grouped:  # (it would also change the rule: a grouped trainer is never plain)
            raise ValueError("decay groups are switched on or off at construction (build a new trainer)")
        if (new.adamw, new.plain) != (self.opt.adamw, self.opt.plain):
            raise ValueError("the optimizer rule is fixed at construction (build a new trainer)")
        if new.emas != self.opt.emas:
            raise ValueError("the weight EMA is switched on or off at construction (build a new trainer)")
        if new.clips and self.xgmi is not None:
            raise ValueError("gradient clipping is not available with the xGMI exchange")
        self.opt = new
        self.lr, self.momentum, self.weight_decay = new.lr, new.momentum, new.weight_decay
        self._opt_tables()
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
        # decay groups: the biases' own weight decay, through the grouped entry points (the MLP has no
        # normalisation layer, so norm_weight_decay has nothing to act on)
        gsfx, gargs = ("_groups", (self.opt.decays()[2],)) if self.opt.grouped else ("", ())
        # the update kernel's three forms: the fused "sgd" (the slab reduced and applied), the "reduce"
        # of the slab into grad (rule-independent; no cursor bump) and the "update" from grad
        for name, from_grad in (("sgd", False), ("reduce", False), ("update", True)):
            slab, gin = (None, p(self.grad)) if from_grad else (p(self.slab), None)
            reduce = name == "reduce"
            if not reduce and not self.opt.plain:  # under a step-counter rule
                lc[name] = n.Launch("sl_mlp_opt" + gsfx, self.opt.rule, p(self.params), p(self.mom), p(self.v),
                                    slab, self.slices, self.slab_stride, gin, self.lr, self.momentum,
                                    self.weight_decay, *self.dw1_coeffs, *ws, p(self.cursor), p(self.r1p),
                                    *self._opt_args(), *gargs)
                continue
            lc[name] = n.Launch("sl_mlp_sgd", p(self.params), p(self.mom), slab, self.slices, self.slab_stride,
                                gin, p(self.grad) if reduce else None, self.lr, self.momentum, self.weight_decay,
                                *self.dw1_coeffs, 1 if reduce else 2, *ws, None if reduce else p(self.cursor),
                                p(self.r1p))
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
                lc["xupdate"] = n.Launch("sl_mlp_opt_xgmi" + gsfx, self.opt.rule, p(self.params), p(self.mom), p(self.v),
                                         self.lr, self.momentum, self.weight_decay, *ws, p(self.cursor), *xg.args(),
                                         p(self.r1p), xg.inline_sync, *self._opt_args(), *gargs)
        self._lc, self._lkey = lc, key
        return lc

    def _opt_args(self) -> tuple:
        """Trailing arguments of sl_mlp_opt / sl_mlp_opt_xgmi: step, ticket, lr table, Adam scalars."""
        p = self._n.ptr
        return (p(self.opt_step), p(self.opt_ticket), p(self.lr_tab),
                self.lr_tab.numel() if self.lr_tab is not None else 0, *self.opt.adam_scalars())

    def _eval_rows(self, s: dict, x, y, rows: int, loss=None, correct=None, logits=None, cursor=None,
                   n_batches: int = 1) -> None:
        """The evaluation-form rows launch (forward only) on the weight set ``s`` (:meth:`_eval_set`):
        ``rows`` rows of (x, y) -- batch ``cursor % n_batches`` of them with a device cursor -- into
        whichever of the per-row ``loss`` / ``correct`` and the ``logits`` are given."""
        n = self._n
        p = n.ptr
        n.call("sl_mlp_rows", p(x), p(y), p(cursor), n_batches, rows,
               p(s["w1h"]), p(s["w2h"]), p(s["w3h"]), p(s["w2th"]), p(s["w3th"]),
               p(s["params"]), self.xa, self.xb, 1.0, 1.0, None, None, None, None,
               p(loss), p(correct), p(logits), 0, p(s["r1p"]), None, n.stream_ptr())

    def _rows(self, train: bool = True):
        if train:
            return self._launches()["rows"]()
        self._eval_rows(self._eval_set(False), self.x, self.y, self.batch, self.loss, self.correct,
                        cursor=self.cursor, n_batches=self.n_batches)

    def _wgrad(self):
        self._launches()["wgrad"]()

    def _sgd(self, mode: int, from_grad: bool, grad_out: bool, bump: bool = True):
        """(tests, scripts) An update-kernel launch by its form: "reduce" writes the gradient out,
        "update" reads it, "sgd" does neither."""
        self._launches()["reduce" if grad_out else "update" if from_grad else "sgd"]()

    def compute_grads(self) -> torch.Tensor:
        """Forward + backward only; returns the reduced (local) gradient (not with an xGMI
        exchange enabled: its rows launch advances the exchange's step id)."""
        lc = self._launches()
        lc["rows"]()
        lc["wgrad"]()
        lc["reduce"]()
        return self.grad[:N_PARAMS]

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
        """One step.  Of ``accum_steps`` > 1 micro-batches: grad = ((g_0 + g_1) + ...) + g_last, then
        the reduce -> hook -> clip -> update path of a clipping step (no fused slab update)."""
        if getattr(self, "probe", None) is not None:
            self.probe()
        lc, ph, last = self._launches(), self.phases, self.accum_steps - 1
        for i in range(last + 1):
            lc["rows"]()
            lc["wgrad"]()
            if last:
                lc["reduce"]()
                for launch in lc["acc_fold" if i == last else "acc_add" if i else "acc_store"]:
                    launch()
                if i < last:
                    lc["bump"]()
        ph.mark("compute")
        if self.xgmi is not None:  # (never with accumulation)
            lc["xreduce"]()
            for launch in lc["xbarrier"]:
                launch()
            ph.mark("exchange")  # slab reduction into the exchange slot + the step barrier(s)
            lc["xupdate"]()      # (the peers' slots are summed inside the update kernel)
        elif self.allreduce is None and not self.opt.clips and not last:
            lc["sgd"]()
        else:
            if not last:
                lc["reduce"]()
            if self.allreduce is not None:
                self.allreduce(self.grad)
                ph.mark("exchange")
            if self.opt.clips:  # the whole norm before any weight moves: the fused slab update cannot clip
                lc["clip"]()
            lc["update"]()
        if self.ema is not None:  # local, so also behind the xGMI update
            lc["ema"]()
        ph.mark("update")

    def probe_step(self):
        """One eager training step with its phase boundaries recorded (utils/phases.py): returns
        a PendingPhases (resolved by the caller once the device has finished the step) carrying
        the gradient payload aggregated per step (fp32 bytes, 0 at world 1)."""
        self.phases.arm()
        self._step_eager()
        pending = self.phases.finish()
        pending.exchange_bytes = 4 * N_PARAMS if (self.allreduce is not None or self.xgmi is not None) else 0
        return pending

    def capture(self, warmup: int = 2, unroll: int = 1) -> None:
        """:meth:`GraphedStep.capture`; ``unroll > 1`` also captures a k-step graph used by :meth:`steps`."""
        super().capture(warmup)
        self.graph_unrolled, self.unroll = None, max(1, int(unroll))
        if self.unroll > 1:
            self.graph_unrolled = self._capture_steps(self.unroll)

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

    def _eval_set(self, ema: bool) -> dict:
        """The weights an evaluation launch reads: the training set, or with ``ema`` a second set
        of shadows (allocated on first use) rebuilt from the averaged parameters by the launch that
        ``refresh_shadows`` uses -- what a second trainer holds after ``set_flat(ema_flat())``.  No
        training tensor is written or moved, so a captured graph stays valid."""
        if not ema:
            return dict({k: getattr(self, k) for k in self.SHADOWS}, params=self.params)
        if self.ema is None:
            raise ValueError("ema=True: this trainer keeps no weight EMA (ema_decay=0)")
        if self._ema_eval is None:
            self._ema_eval = {k: torch.zeros_like(getattr(self, k)) for k in self.SHADOWS}
        self._build_shadows(self.ema, self._ema_eval)
        return dict(self._ema_eval, params=self.ema)

    def evaluate(self, x_u8: torch.Tensor, y_u8: torch.Tensor, ema: bool = False) -> StepStats:
        """Mean loss / accuracy over the whole 64-row blocks of (x, y); ``ema=True``: of the
        averaged parameters, the training state untouched (between steps)."""
        s = self._eval_set(ema)
        x = x_u8.reshape(-1, D_IN).to(self.device).contiguous()
        y = y_u8.reshape(-1).to(self.device).to(torch.uint8).contiguous()
        rows = x.shape[0] // BLOCK_ROWS * BLOCK_ROWS
        loss = torch.zeros(rows, device=self.device)
        corr = torch.zeros(rows, device=self.device)
        self._eval_rows(s, x, y, rows, loss, corr)
        lv = float("nan") if int(s["r1p"].max()) >= R1_OVF_MIN else float(loss.mean())
        return StepStats(lv, float(corr.mean()), rows)

    def logits(self, x_u8: torch.Tensor, ema: bool = False) -> torch.Tensor:
        s = self._eval_set(ema)
        x = x_u8.reshape(-1, D_IN).to(self.device).contiguous()
        rows = x.shape[0]
        if rows % BLOCK_ROWS:
            raise ValueError(f"rows must be a multiple of {BLOCK_ROWS}")
        out = torch.empty(rows, CLASSES, device=self.device)
        self._eval_rows(s, x, None, rows, logits=out)
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
        self._eval_rows(s, xp, yp, rows, loss, logits=out)
        E.eval_accum(out, yp, loss, N, CLASSES, topk, acc)
        rep = E.report_from_acc(acc, CLASSES, topk)
        return rep.all_bad() if int(s["r1p"].max()) >= R1_OVF_MIN else rep

    def get_flat(self) -> torch.Tensor:
        return self.params[:N_PARAMS].clone()

    def set_flat(self, flat: torch.Tensor) -> None:
        self.params[:N_PARAMS].copy_(flat.to(self.params))
        self.refresh_shadows()
