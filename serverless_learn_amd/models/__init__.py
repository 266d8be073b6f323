"""Model registry: the worker asks for a trainer by name (``Config.model``).

Every trainer exposes the same interface, so the runtime (gossip, parameter
server, all-reduce DP, checkpoints) is model-agnostic: everything travels as
one flat parameter vector, exactly what the reference's ``Update{repeated
double delta}`` carries (proto :81-83).  All four trainers provide:

* the model: ``n_params``, ``model_name``, ``layout``, ``batch``;
* data and the step: ``load_shard``, ``step``, ``probe_step`` (one step with
  its phases timed), ``stats``, ``allreduce`` (gradient hook);
* parameters: ``params`` / ``mom`` (flat fp32 vectors), ``get_flat`` /
  ``set_flat``, ``refresh_shadows``, ``ema`` / ``ema_flat`` (the weight EMA);
* the group: ``set_world``, ``set_accum``, ``accum_steps``,
  ``samples_per_step``, ``buffers`` (state a regroup broadcasts beside
  params / mom);
* checkpoints: ``opt`` (``opt.meta()``), ``state_extra`` /
  ``load_state_extra``, ``reset_optimizer_state``;
* reporting: ``grad_norm``, ``evaluate``, ``evaluate_full``.

What does not depend on the model -- optimizer, EMA and accumulation state,
its checkpoint form and ``buffers()`` order -- is written once, in
:mod:`.trainer_state`.  The GPU engines add ``capture`` / ``drop_graphs``
(utils/graphs.py), the MLP engine ``steps`` and ``enable_xgmi``, the ResNet
engine ``bucket_hook`` / ``bucket_wait``; the worker asks before it uses those.
"""
from __future__ import annotations

import torch

MODELS = ("mlp", "resnet18")


def make_trainer(model: str, device: torch.device, **kw):
    """A GPU (hand-written HIP kernels) or CPU (torch reference) trainer."""
    cuda = torch.device(device).type == "cuda"
    if model == "mlp":
        from . import mlp

        return mlp.FusedMLPTrainer(device=device, **kw) if cuda else mlp.CPUTrainer(**kw)
    if model in ("resnet18", "resnet18-cifar"):
        from . import resnet

        if cuda:
            from .resnet_engine import FusedResNetTrainer

            return FusedResNetTrainer(device=device, **kw)
        return resnet.CPUResNetTrainer(**kw)
    raise ValueError(f"unknown model {model!r} (choose from {MODELS})")
