"""Typed runtime configuration.

The reference is configured only at compile time: ``#define``s in
/root/reference/src/serverless_learn.h:5-12 (addresses, gossip and simulated
training intervals), file constants in /root/reference/src/master.cc:43,46,60
(push/checkup intervals, LEARN_RATE) and /root/reference/src/file_server.cc:40,46
(dummy file and chunk size); the only runtime flag is the worker's argv[1]
(/root/reference/src/worker.cc:234-239).

Here every knob is a dataclass field whose DEFAULT EQUALS THE REFERENCE
CONSTANT, overridable by ``SL_<FIELD>`` environment variables and by CLI flags
(:func:`add_cli_args` / :func:`from_args`).
"""
from __future__ import annotations

import argparse
import dataclasses
import math
import os
from dataclasses import dataclass, field


@dataclass
class Config:
    # --- well-known endpoints (serverless_learn.h:5,8) ---
    master_addr: str = "localhost:50052"
    file_server_addr: str = "localhost:50053"
    # --- cadences, milliseconds (serverless_learn.h:10,12; master.cc:43,46) ---
    gossip_interval_ms: int = 5000
    simulated_train_interval_ms: int = 2000
    push_interval_ms: int = 5000
    checkup_interval_ms: int = 5000
    ps_broadcast_interval_ms: int = 0  # master -> random worker PS exchange (master.cc:268-293, never
                                       # started in the reference; it would run every 5000 ms); 0 = off
    # --- learning constants (master.cc:60) ---
    learn_rate: float = 0.5            # gossip / PS mixing coefficient alpha
    # --- data plane (file_server.cc:40,46) ---
    chunk_size: int = 1_000_000
    dummy_file_length: int = 100_000_000
    dataset: str = "synthetic-mnist"   # | "synthetic-cifar" | "synthetic-cifar100" (100 classes, resnet18) |
                                       # "reference-dummy" (byte-exact reference file 0)
    shard_records: int = 127_388       # records per shard: a 100,000,000-byte shard
    num_shards: int = 0                # 0 = one shard per worker
    push_policy: str = "on_change"     # "on_change" | "periodic" (reference: re-push every interval)
    store_dir: str = ""                # persist uploaded checkpoints here (file server)
    # --- failure detection / transport (new; reference has none) ---
    rpc_timeout_s: float = 5.0
    max_misses: int = 3                # evict after this many failed heartbeats
    max_message_bytes: int = 256 << 20
    rendezvous_port: int = 0           # master's collective rendezvous store (0 = pick free)
    metrics_port: int = 0              # > 0: serve Prometheus /metrics on this port (0 = off)
    # --- worker training ---
    sync: str = "allreduce"            # allreduce | gossip | ps | none
    gossip_compat: bool = False        # reproduce the reference's alpha^2 echo exactly
    gossip_topk: float = 0.0           # sync=gossip: send only this fraction of the parameters per message, the
                                       # largest |m - o| (0 = dense; 0 < x <= 1; not with ps / simulate / compat)
    device: str = "auto"               # auto | cpu | cuda[:N]
    model: str = "mlp"                 # mlp | resnet18 | simulate (reference: vector += 1)
    classes: int = 0                   # resnet18: outputs of the classifier head (1..256); 0 = the dataset's own
                                       # count, 10 or synthetic-cifar100's 100.  mlp / simulate: 0 or 10
    batch: int = 1024
    lr: float = 0.05
    momentum: float = 0.9
    weight_decay: float = 0.0
    norm_weight_decay: float = -1.0    # resnet18: weight decay of the BatchNorm scales and shifts; -1 = weight_decay
    bias_weight_decay: float = -1.0    # weight decay of the other biases (fc.bias; the MLP's b1 b2 b3); -1 = weight_decay
    optimizer: str = "sgd"             # sgd (momentum SGD) | adamw (beta1, beta2, adam_eps; decoupled weight_decay)
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1e-8
    lr_schedule: str = "constant"      # constant | linear | cosine: what follows the warm-up (ops/optim.py lr_at)
    lr_warmup_steps: int = 0           # linear warm-up over this many steps (0 = none)
    lr_decay_steps: int = 0            # step at which the decay ends (0 = max_steps)
    lr_min_ratio: float = 0.0          # the decay ends at lr_min_ratio * lr
    clip_grad_norm: float = 0.0        # clip the aggregated gradient to this global L2 norm (0 = off, inf = measure)
    accum_steps: int = 1               # micro-batches per optimizer step (one exchange, one clip, one update)
    global_batch: int = 0              # > 0: accum_steps is chosen at every membership change so that
                                       # accum_steps * batch * world is as close to this as it can be (0 = off)
    ema_decay: float = 0.0             # > 0: keep an exponential moving average of the weights, updated after every
                                       # optimizer step (0 = off; < 1)
    ema_warmup: bool = True            # decay_t = min(ema_decay, (1 + t) / (10 + t)): early updates weigh more
    augment: str = "none"              # resnet18: none | crop-flip (random crop + horizontal flip, data/augment.py)
    augment_pad: int = 4               # crop-flip: black pixels of padding around the image the crop is taken from
    shuffle: bool = False              # resnet18: draw each epoch's records through a fresh permutation of the shard
    label_smoothing: float = 0.0       # resnet18: smooth the training targets by this much (0 <= eps < 1)
    mixup_alpha: float = 0.0           # resnet18: mixup with lambda ~ Beta(alpha, alpha) per batch (0 = off)
    cutmix_alpha: float = 0.0          # resnet18: CutMix likewise; with both on, one of the two per batch
    seed: int = 0
    eval_every: int = 0                # > 0: every this many steps, evaluate on the held-out shard (file EVAL_BASE,
                                       # pushed once per worker); 0 = off
    eval_records: int = 10_000         # records of the held-out shard (1..2^22)
    eval_topk: int = 5                 # the k of the reported top-k accuracy (1..10)
    eval_seed: int = -1                # seed of the held-out records; -1 = seed + 1 (never equal to seed)
    checkpoint_every: int = 0          # steps between checkpoints (rank 0); 0 = off
    max_steps: int = 0                 # 0 = run until stopped
    log_every: int = 50
    graph: bool = True                 # capture the fused step in a hipGraph when possible
    graph_steps: int = 16              # steps per graph replay chunk (error / metrics checks between chunks)
    graph_collectives: bool = False    # also capture a multi-rank RCCL group's collectives into the step graph
    dp_backend: str = "auto"           # auto (nccl = RCCL on GPU, gloo on CPU) | nccl | gloo
    dp_timeout_s: float = 30.0         # collective / rendezvous timeout of the data-parallel group
    xgmi: bool = True                  # MLP on a GPU group: all-reduce through IPC-mapped buffers over xGMI
    extra: dict = field(default_factory=dict)

    @classmethod
    def from_env(cls, **overrides) -> "Config":
        cfg = cls()
        for f in dataclasses.fields(cls):
            key = "SL_" + f.name.upper()
            if key in os.environ and f.name != "extra":
                setattr(cfg, f.name, _coerce(f, os.environ[key]))
        for k, v in overrides.items():
            setattr(cfg, k, v)
        cfg.validate()
        return cfg

    def __post_init__(self):
        self.validate()

    def validate(self) -> None:
        """Refuse combinations no component implements (gradient accumulation's, the weight EMA's,
        the decay groups', the input pipeline's, the soft-target loss's, held-out evaluation's and the
        top-k sparse gossip's)."""
        self._validate_eval()
        self._validate_classes()
        self._validate_decay_groups()
        if isinstance(self.accum_steps, bool) or int(self.accum_steps) != self.accum_steps or self.accum_steps < 1:
            raise ValueError(f"accum_steps must be an integer >= 1, got {self.accum_steps!r}")
        if isinstance(self.global_batch, bool) or int(self.global_batch) != self.global_batch or self.global_batch < 0:
            raise ValueError(f"global_batch must be an integer >= 0 (0 = off), got {self.global_batch!r}")
        if self.global_batch > 0 and self.accum_steps != 1:
            raise ValueError("accum_steps and global_batch: set one of them (global_batch chooses accum_steps)")
        if 0 < self.global_batch < self.batch:
            raise ValueError(f"global_batch {self.global_batch} is smaller than one worker's batch {self.batch}")
        if (self.accum_steps != 1 or self.global_batch > 0) and self.model == "simulate":
            raise ValueError("accum_steps / global_batch: the simulate model has no gradient to accumulate")
        if self.ema_decay != 0:  # NaN included
            from .ops.optim import ema_table_len

            ema_table_len(self.ema_decay, self.ema_warmup)  # a bad decay, a warm-up table that is too long
            if self.model == "simulate":
                raise ValueError("ema_decay: the simulate model has no trained weights to average")
        if (self.augment, self.augment_pad, self.shuffle) != ("none", 4, False) and self.model in ("mlp", "simulate"):
            # the MLP kernels read X from bricks tiled once per shard: a per-sample gather would undo that
            raise ValueError(f"augment / shuffle: the {self.model} model has no input pipeline (model='resnet18')")
        if (self.label_smoothing, self.mixup_alpha, self.cutmix_alpha) != (0, 0, 0):  # NaN included
            from .data.augment import check_mix

            check_mix(self.label_smoothing, self.mixup_alpha, self.cutmix_alpha)
            if self.model in ("mlp", "simulate"):
                # the MLP rows kernel fuses its own one-hot loss and reads X from bricks tiled once per shard
                raise ValueError(f"label_smoothing / mixup_alpha / cutmix_alpha: the {self.model} model has neither "
                                 "a soft-target loss nor an input pipeline (model='resnet18')")
        x = self.gossip_topk
        if x == 0:
            return
        if not 0 < x <= 1:  # NaN included
            raise ValueError(f"gossip_topk must be 0 (dense) or a fraction in (0, 1], got {x!r}")
        if self.sync == "ps":
            raise ValueError("gossip_topk: the master's parameter server stays dense (sync='ps')")
        if self.model == "simulate":
            raise ValueError("gossip_topk: the simulate model is growable and is never sparse")
        if self.gossip_compat:
            raise ValueError("gossip_topk: gossip_compat reproduces the reference's dense exchange byte for byte")

    def _validate_decay_groups(self) -> None:
        for name in ("norm_weight_decay", "bias_weight_decay"):
            v = getattr(self, name)
            if v == -1:
                continue
            if isinstance(v, bool) or not (math.isfinite(v) and v >= 0):  # NaN included
                raise ValueError(f"{name} must be -1 (follow weight_decay) or a finite number >= 0, got {v!r}")
            if self.model == "simulate":
                raise ValueError(f"{name}: the simulate model has no optimizer")
        if self.norm_weight_decay != -1 and self.model == "mlp":
            raise ValueError("norm_weight_decay: the mlp model has no normalisation layer (model='resnet18')")

    @property
    def decay_groups(self) -> dict:
        """The trainers' ``norm_weight_decay=`` / ``bias_weight_decay=`` keywords: those that are set
        (-1 is None, the trainers' "follow weight_decay", and is left out)."""
        return {k: float(getattr(self, k)) for k in ("norm_weight_decay", "bias_weight_decay") if getattr(self, k) != -1}

    def _validate_classes(self) -> None:
        v = self.classes
        if isinstance(v, bool) or int(v) != v or not 0 <= v <= 256:
            raise ValueError(f"classes must be an integer in 0..256 (0 = the dataset's own count), got {v!r}")
        if self.model in ("mlp", "simulate"):
            # the MLP rows kernel fuses a 10-wide loss; the simulate model has no classifier
            if v not in (0, 10):
                raise ValueError(f"classes={v}: the {self.model} model has ten classes (model='resnet18')")
            if self.dataset == "synthetic-cifar100":
                raise ValueError(f"dataset synthetic-cifar100 has 100 classes: the {self.model} model has ten "
                                 "(model='resnet18')")

    @property
    def n_classes(self) -> int:
        """The classifier head's outputs: ``classes``, or with 0 the dataset's own count."""
        if self.classes:
            return int(self.classes)
        from .data.device_synth import dataset_classes

        return dataset_classes(self.dataset)

    def _validate_eval(self) -> None:
        def integer(name, lo, hi=None):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or v < lo or (hi is not None and v > hi):
                rng = f"in {lo}..{hi}" if hi is not None else f">= {lo}"
                raise ValueError(f"{name} must be an integer {rng}, got {v!r}")

        integer("eval_every", 0)
        integer("eval_records", 1, 1 << 22)  # (the int64 loss sum of ops/evalmetrics.py holds that many)
        integer("eval_topk", 1, 10)
        if self.held_out_seed == self.seed:
            raise ValueError(f"eval_seed {self.eval_seed} equals seed: the held-out records would be training records")
        if self.eval_every > 0 and self.model == "simulate":
            raise ValueError("eval_every: the simulate model has nothing to evaluate")
        if self.eval_every > 0 and self.dataset == "reference-dummy":
            raise ValueError("eval_every: the reference-dummy dataset has no held-out set")

    @property
    def held_out_seed(self) -> int:
        """The seed of the held-out shard's records: ``eval_seed``, by default ``seed + 1`` (the field
        stays -1, so a later change of ``seed`` moves it along)."""
        return self.seed + 1 if self.eval_seed == -1 else self.eval_seed

    def accum_for(self, world: int) -> int:
        """Micro-batches per step in a lock-step group of ``world`` workers: ``accum_steps``, or with
        a ``global_batch`` G the K whose ``K * batch * world`` is nearest to G, ``max(1, floor(G /
        (batch * world) + 1/2))``.  Every member derives it from the same view, so a group agrees
        without a collective."""
        if self.global_batch <= 0:
            return self.accum_steps
        per = self.batch * max(1, int(world))
        return max(1, (2 * self.global_batch + per) // (2 * per))  # floor(G / per + 1/2), in integers

    def gossip_k(self, n: int) -> int:
        """Entries per sparse message for an n-parameter model (0 = dense)."""
        return max(1, math.ceil(self.gossip_topk * n)) if self.gossip_topk > 0 else 0

    @property
    def gossip_interval(self) -> float:
        return self.gossip_interval_ms / 1000.0

    @property
    def push_interval(self) -> float:
        return self.push_interval_ms / 1000.0

    @property
    def ps_broadcast_interval(self) -> float:
        return self.ps_broadcast_interval_ms / 1000.0

    @property
    def checkup_interval(self) -> float:
        return self.checkup_interval_ms / 1000.0


def _coerce(f, raw: str):
    t = f.type if isinstance(f.type, type) else {"int": int, "float": float, "bool": bool, "str": str}.get(str(f.type), str)
    if t is bool:
        return raw.strip().lower() in ("1", "true", "yes", "on")
    return t(raw)


def add_cli_args(ap: argparse.ArgumentParser, only=None) -> None:
    for f in dataclasses.fields(Config):
        if f.name == "extra" or (only is not None and f.name not in only):
            continue
        flag = "--" + f.name.replace("_", "-")
        if f.type in (bool, "bool"):
            ap.add_argument(flag, type=lambda s: s.lower() in ("1", "true", "yes", "on"), default=None)
        else:
            t = {"int": int, "float": float, "str": str}.get(str(f.type), f.type if isinstance(f.type, type) else str)
            ap.add_argument(flag, type=t, default=None)


def from_args(args: argparse.Namespace) -> Config:
    cfg = Config.from_env()
    for f in dataclasses.fields(Config):
        v = getattr(args, f.name, None)
        if v is not None:
            setattr(cfg, f.name, v)
    cfg.validate()
    return cfg
