"""What the four trainers share, whatever the model: optimizer, weight-EMA and gradient-accumulation
state with its checkpoint form, and the CPU trainers' step.

:class:`TrainerState` is mixed into ``CPUTrainer``, ``CPUResNetTrainer``, ``FusedMLPTrainer`` and
``FusedResNetTrainer``; the checkpoint keys and the order of ``buffers()`` (what a regroup
broadcasts) are therefore the same on all of them by construction.  Its ``_opt_update`` and
``_accumulate`` are the CPU reference: the definitions the GPU engines are tested against.
:class:`CPUTrainerBase` adds the step the two CPU trainers run on top of them.  (The GPU engines'
``step`` / ``capture`` / ``drop_graphs`` live beside the graph slots, utils/graphs.py.)
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ..ops.optim import (ACCUM_KERNELS, CLIP_KERNELS, EMA_KERNELS, OptSpec, check_accum_steps, clip_buffers,
                         clip_grad_, decay_vector, ema_update_, require_kernels, sgd_update, trainer_class_map)


@dataclass
class StepStats:
    loss: float
    accuracy: float
    samples: int

    @property
    def n(self) -> int:
        """Samples behind ``loss`` / ``accuracy`` (a training step's: ``accum_steps * batch``)."""
        return self.samples


class TrainerState:
    """Optimizer state of a trainer beyond ``params``: the momentum ``mom``, AdamW's second moment
    ``v`` and the optimizer step ``opt_step`` (a 1-element tensor, so a regroup broadcasts it with
    the rest), each only where the rule needs it; with ``ema_decay > 0`` the averaged parameters
    ``ema``, their update count ``ema_step`` and the coefficient table ``ema_tab`` (ops/optim.py
    ema_table).  All of it lives on ``self.device``; on a GPU also the schedule's table ``lr_tab``,
    gradient clipping's scratch, gradient accumulation's partial sums and the ticket words the
    owner's launches use (:attr:`tickets`).  This class is the weight EMA's definition on the
    trainers.

    With decay groups on (``norm_weight_decay`` / ``bias_weight_decay``, ops/optim.py) also
    ``decay_cls``, the class of every 64-element block of ``params`` (a uint8 tensor on
    ``self.device``), and on the CPU ``decay_vec``, the float64 decay of every element that the
    reference update takes.  Both follow from the model and the hyper-parameters: they are no
    state, and a trainer without groups has neither attribute.

    The owner sets ``params`` (``n_params`` real entries, then any padding) before
    :meth:`_init_state`, and keeps ``cursor`` (an int, or a 1-element tensor on the device)."""

    device = torch.device("cpu")
    tickets = ()                  # of "opt_ticket" / "ema_ticket": the words the owner's launches use
    opt_kernels = ()              # entry points of the owner's step-counter rules
    group_kernels = ()            # ... and of those rules with decay groups on
    accum_kernels = ACCUM_KERNELS  # ... and of its accumulated step
    graph = None                  # a captured step (GPU engines: a slot of utils/graphs.py)
    grad = None                   # the aggregated gradient of the last step, as the optimizer took it
    acc = loss_acc = correct_acc = None  # GPU: an accumulated step's partial sums (None at accum_steps 1)

    def _init_state(self, batch: int, lr: float, momentum: float, weight_decay: float, world_size: int,
                    accum_steps: int, opt: dict) -> None:
        """``opt``: optimizer=, beta1=, beta2=, adam_eps=, lr_schedule=, lr_warmup_steps=, ... (OptSpec)."""
        self.batch = batch
        self.lr, self.momentum, self.weight_decay = lr, momentum, weight_decay
        self.world_size = world_size
        # accum_steps micro-batches per optimizer step: the gradient stays a mean over all of them
        self.accum_steps = check_accum_steps(accum_steps)
        self.opt = spec = OptSpec(lr=lr, momentum=momentum, weight_decay=weight_decay, **opt)
        word = lambda: torch.zeros(1, dtype=torch.int32, device=self.device)  # noqa: E731
        self.mom = torch.zeros_like(self.params) if (momentum > 0 or spec.adamw) else None
        # AdamW's second moment (mom is its first); the optimizer step the update reads (and the
        # ticket word of a launch that advances it itself) where the rule depends on the step
        self.v = torch.zeros_like(self.params) if spec.adamw else None
        self.opt_step = self.opt_ticket = self.lr_tab = None
        if not spec.plain:
            if self._gpu:
                require_kernels(spec, *(self.group_kernels if spec.grouped else self.opt_kernels))
            self.opt_step = word()
            self.opt_ticket = word() if "opt_ticket" in self.tickets else None
        self.clip_partials = self.clip_norm = self._grad_norm = None
        # the weight EMA: it starts at the initial parameters (flat= included)
        self.ema = self.ema_step = self.ema_ticket = self.ema_tab = None
        if spec.emas:
            if self._gpu:
                require_kernels(spec, *EMA_KERNELS)
            self.ema = self.params.clone()
            self.ema_step = word()
            self.ema_ticket = word() if "ema_ticket" in self.tickets else None
        if spec.grouped:  # built once: the layout does not change
            self.decay_cls = torch.from_numpy(trainer_class_map(self)).to(self.device)
        self._opt_tables()

    def norm_tensors(self) -> tuple:
        """Names (as in ``layout()``) of the normalisation layers' tensors: decay class 1."""
        return ()

    @property
    def _gpu(self) -> bool:
        return self.device.type == "cuda"

    def _opt_tables(self) -> None:
        """What follows ``self.opt``'s hyper-parameters: the EMA's coefficients and, for the kernels,
        the learning-rate table and gradient clipping's scratch (the workgroups' fp64 partial sums
        and the norm it reports)."""
        spec = self.opt
        if spec.emas:
            self.ema_tab = torch.from_numpy(spec.ema_table()).to(self.device)
        if spec.grouped and not self._gpu:
            self.decay_vec = decay_vector(self.decay_cls.numpy(), self.params.numel(), spec.decays())
        if not self._gpu:
            return
        if not spec.plain:
            tab = spec.lr_table()
            self.lr_tab = torch.from_numpy(tab).to(self.device) if tab is not None else None
        if spec.clips and self.clip_norm is None:
            require_kernels(spec, *CLIP_KERNELS)
            self.clip_partials, self.clip_norm = clip_buffers(self.n_params, self.device)

    # ---- the CPU reference update: the definition the GPU engines are tested against ----
    def _opt_update(self, g: torch.Tensor) -> None:
        if self.opt.clips:
            self._grad_norm = clip_grad_(g, self.opt.clip_grad_norm)
        if self.opt_step is None:
            sgd_update(self.params, self.mom, g, self.lr, self.momentum, self.weight_decay)
        else:
            self.opt.update(self.params, self.mom, self.v, g, int(self.opt_step[0]),
                            self.decay_vec if self.opt.grouped else None)
            self.opt_step += 1
        if self.ema is not None:  # once per update, on the parameters just written
            t = min(int(self.ema_step[0]), self.ema_tab.numel() - 1)
            ema_update_(self.ema, self.params, self.ema_tab[t])
            self.ema_step += 1

    def grad_norm(self) -> float | None:
        """The aggregated gradient's global L2 norm at the last step, before clipping (on a GPU one
        float read from the device); None with clipping off, and on the CPU before the first step."""
        if not self.opt.clips or self.clip_norm is None:
            return self._grad_norm
        return float(self.clip_norm[0])

    def ema_flat(self) -> torch.Tensor:
        """A copy of the averaged parameters (``ema_decay > 0``)."""
        if self.ema is None:
            raise ValueError("this trainer keeps no weight EMA (ema_decay=0)")
        return self.ema[:self.n_params].clone()

    # ---- exact-resume state beyond the flat vectors (ckpt format v2) ----
    def _model_extra(self) -> dict:
        """The model's own part of :meth:`state_extra` (BatchNorm running statistics)."""
        return {}

    def state_extra(self) -> dict:
        """The batch cursor: a resumed run continues with the batch the saved run would have taken
        next, so save-at-k + resume + m steps equals k + m steps.  Then the model's own state, the
        optimizer step and AdamW's second moment (the first travels as the momentum section), the
        averaged parameters and the number of EMA updates behind them."""
        c = self.cursor
        d = {"cursor": c.double().cpu().numpy() if torch.is_tensor(c) else np.array([c], dtype=np.float64)}
        d.update(self._model_extra())
        n = self.n_params
        if self.opt_step is not None:
            d["opt_step"] = self.opt_step.double().cpu().numpy()
        if self.v is not None:
            d["exp_avg_sq"] = self.v[:n].double().cpu().numpy()
        if self.ema is not None:
            d["ema"] = self.ema[:n].double().cpu().numpy()
            d["ema_step"] = self.ema_step.double().cpu().numpy()
        return d

    def load_state_extra(self, d: dict) -> None:
        n = self.n_params
        f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)  # noqa: E731
        if "cursor" in d:
            if torch.is_tensor(self.cursor):
                self.cursor.fill_(int(d["cursor"][0]))
            else:
                self.cursor = int(d["cursor"][0])
        if self.opt_step is not None and "opt_step" in d:
            self.opt_step.fill_(int(d["opt_step"][0]))
        if self.v is not None and "exp_avg_sq" in d:
            self.v[:n].copy_(f32(d["exp_avg_sq"]))
        if self.ema is not None:
            if "ema" in d and "ema_step" in d:
                self.ema[:n].copy_(f32(d["ema"]))
                self.ema_step.fill_(int(d["ema_step"][0]))
            else:  # a checkpoint without one: the average starts over from the weights just loaded
                self.ema.copy_(self.params)
                self.ema_step.zero_()
        for t in (self.opt_ticket, self.ema_ticket):  # (a run that died inside a launch may have left one set)
            if t is not None:
                t.zero_()

    def buffers(self) -> list:
        """Optimizer state beyond params / mom (and the weight EMA), broadcast with them after a
        regroup."""
        return [t for t in (self.v, self.opt_step, self.ema, self.ema_step) if t is not None]

    def reset_optimizer_state(self) -> None:
        for t in (self.mom, self.v, self.opt_step, self.opt_ticket):
            if t is not None:
                t.zero_()

    # ---- gradient accumulation and the group size ----
    @property
    def samples_per_step(self) -> int:
        return self.batch * self.accum_steps

    @property
    def grad_scale(self) -> float:
        """The gradient is a mean over the global batch ``batch * world_size * accum_steps``."""
        return 1.0 / (self.batch * self.world_size * self.accum_steps)

    def set_world(self, world: int) -> None:
        """The gradient scale follows the group size; a captured step holds the old one."""
        self.world_size = world
        self.graph = None

    def _alloc_accum(self) -> None:
        """GPU: the partial sums of an accumulated step (gradient, per-sample loss and correct)."""
        if self.accum_steps == 1:
            self.acc = self.loss_acc = self.correct_acc = None
        elif self.acc is None and self._gpu:
            require_kernels(self.opt, *self.accum_kernels)
            self.acc = torch.zeros_like(self.grad)
            self.loss_acc, self.correct_acc = torch.zeros_like(self.loss), torch.zeros_like(self.correct)

    def set_accum(self, k) -> None:
        """``k`` micro-batches per optimizer step, each on its own batch (the cursor moves after
        each): their gradients are summed in fp32 in order, and the sum takes one exchange, one clip
        and one update.  The gradient scale follows (a mean over ``k * batch * world``) and a
        captured step is dropped."""
        self.accum_steps = check_accum_steps(k)
        self._alloc_accum()
        self.set_world(self.world_size)

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


class CPUTrainerBase(TrainerState):
    """The plain-torch trainers' step over the reference update: a subclass gives ``_micro`` (the
    micro-batch at the cursor), ``load_shard`` and ``evaluate*``."""

    def _init_cpu(self, flat: torch.Tensor, *state) -> None:
        """``state``: :meth:`TrainerState._init_state`'s arguments."""
        from ..utils.phases import PhaseProbe

        self.params = flat.clone().float()
        self._init_state(*state)
        self.cursor = 0
        self.x = self.y = None
        self.allreduce = None  # callable(tensor) -> None (sum in place)
        self._last = None
        self.phases = PhaseProbe("cpu")

    def refresh_shadows(self) -> None:
        pass

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

    def _eval_weights(self, ema: bool) -> torch.Tensor:
        """What ``evaluate(ema=...)`` runs on: the parameters or their average (only read)."""
        if ema and self.ema is None:
            raise ValueError("evaluate(ema=True): this trainer keeps no weight EMA (ema_decay=0)")
        return self.ema if ema else self.params

    def get_flat(self) -> torch.Tensor:
        return self.params.clone()

    def set_flat(self, flat: torch.Tensor) -> None:
        self.params.copy_(flat.to(self.params))
