"""MI355X training engine for the ResNet-18-shaped CNN (BASELINE config 4).

A static execution plan, not an autograd graph: every activation, gradient
and statistics buffer is allocated once for the fixed per-GPU batch, and a
step is a fixed sequence of hand-written HIP kernels (csrc/kernels/conv.hip,
cnn_aux.hip, elementwise.hip) -- so it can be captured whole in a hipGraph
and replayed with zero host work (the data batch is chosen by a device-side
cursor, like the MLP engine).

Per step:
  forward   input_norm (input_aug with shuffle= / augment= on, input_mix with mixup_alpha= /
            cutmix_alpha= on: data/augment.py) ->
            [conv (+BN stats in the epilogue) -> bn_apply with
            the finalize folded in (+residual, ReLU)] x 20 -> avgpool -> fc ->
            softmax-CE (loss, dlogits, dbias; against soft targets with a mix or
            label_smoothing= on); a 64-channel block's conv2 applies
            relu(bn1(.)) while loading c1 instead (BN-on-load, no a1 pass)
  backward  per block, in reverse: bn_bwd_apply (ReLU mask fused), conv wgrad
            (split-K partials in a slab + one ordered reduce into the flat
            gradient) and dgrad, whose epilogue adds the residual gradient,
            applies the next BN's ReLU mask and accumulates that BN's backward
            sums (csrc/kernels/bn_bwd_epi.h), so only the first BN after the
            average pool still needs a bn_bwd_reduce pass (SL_BNB_FUSE=0: one
            per BN, as before)
            (SL_WGRAD_SIDE=1: the split-K slab reduces run on a side stream, forked
            per reduce and joined before the optimizer and each gradient bucket)
  comms     optional: the flat gradient is laid out in forward order, so
            when a block's backward is done its whole parameter range is final
            -> a bucket hook can launch RCCL all-reduce of that range while
            backward continues
  update    one multi-tensor SGD launch over the flat vector (fp32 master,
            momentum, weight decay, bf16 shadow) + one launch that re-lays the
            bf16 conv weights out for dgrad; with ema_decay= on, one launch
            between them that moves the weight EMA towards the new parameters.
"""
from __future__ import annotations

import contextlib
import os
import torch

from ..utils.graphs import GraphedStep
from .resnet import CIFAR_MEAN, CIFAR_STD, BlockSpec, BNSpec, ConvSpec, ResNetModel, init_params, resnet18_spec
from .trainer_state import StepStats, TrainerState

LOGIT_LD = 16  # dlogits row stride up to 16 classes (classes padded for 16-B gathers); above: ops.cnn.logit_ld


class _BN:
    """Per-BatchNorm buffers.  ``stats_buf``/``sums_buf`` are cross-workgroup sum
    buffers (replicas | result | ticket, csrc/kernels/common.h rsum_*) living in
    the per-step zeroed arena; ``stats``/``sums`` are their folded results."""

    def __init__(self, spec: BNSpec, params, grad, arena, off, dev, rs):
        from ..ops import cnn as K

        c = spec.c
        self.spec = spec
        self.gamma = params[spec.g_off:spec.g_off + c]
        self.beta = params[spec.b_off:spec.b_off + c]
        self.ggamma = grad[spec.g_off:spec.g_off + c]
        self.gbeta = grad[spec.b_off:spec.b_off + c]
        self.stats_buf = arena[off:off + rs]
        self.sums_buf = arena[off + rs:off + 2 * rs]
        self.stats = K.rsum_result(self.stats_buf, 2 * c)
        self.sums = K.rsum_result(self.sums_buf, 2 * c)
        self.coef = torch.zeros(4 * c, device=dev)
        self.dcoef = torch.zeros(3 * c, device=dev)
        self.run_mean = torch.zeros(c, device=dev)
        self.run_var = torch.ones(c, device=dev)


class _Conv:
    def __init__(self, spec: ConvSpec, params, shadow, grad, dev, ld_out=None):
        self.spec = spec
        self.w = shadow[spec.off:spec.off + spec.numel]
        self.g = grad[spec.off:spec.off + spec.numel]
        self.ldt = ld_out or spec.cout  # dgrad source channels
        self.wt = torch.zeros(spec.cin * spec.k * spec.k * self.ldt, dtype=torch.bfloat16, device=dev)


class FusedResNetTrainer(ResNetModel, GraphedStep, TrainerState):
    tickets = ("ema_ticket",)  # (the update launches read opt_step; a cursor_bump advances it)
    opt_kernels = ("sl_adamw_flat", "sl_sgd_flat_lr")
    group_kernels = ("sl_adamw_flat_groups", "sl_sgd_flat_lr_groups")

    def __init__(self, batch: int, device="cuda", lr: float = 0.05, momentum: float = 0.9,
                 weight_decay: float = 5e-4, seed: int = 0, world_size: int = 1, stem: str = "cifar",
                 classes: int = 10, flat: torch.Tensor | None = None, bn_momentum: float = 0.1,
                 in_hw: int | None = None, augment: str = "none", augment_pad: int = 4, shuffle: bool = False,
                 label_smoothing: float = 0.0, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0,
                 accum_steps: int = 1, **opt):
        from ..data import augment as A
        from ..ops import _native
        from ..ops import cnn as K
        from ..ops import evalmetrics as E
        from ..ops import optim as O

        # dlogits row stride: LOGIT_LD up to 16 classes (the narrow loss and metrics kernels), else the
        # next power of two >= max(32, classes) (the wide ones); refuses classes outside 1..256
        self.logit_ld = K.logit_ld(classes)
        self.wide = classes > K.NARROW_CLASSES
        self.spec = spec = resnet18_spec(stem, int(classes), in_hw)
        A.check(augment, augment_pad, spec.in_hw)
        A.check_mix(label_smoothing, mixup_alpha, cutmix_alpha, batch)
        _native.lib()
        self.K, self.O, self.E = K, O, E
        self._eval_cache = None  # evaluate_full's padded device copy of the last set passed
        self._ce_kw = {}  # the loss launch's extra arguments: the wide kernel's workspace (set below)
        # the training input pipeline (data/augment.py): a pure function of (seed, cursor, sample),
        # so the cursor that is checkpointed and broadcast already is all the state it has
        self.seed, self.augment, self.augment_pad, self.shuffle = seed, augment, augment_pad, bool(shuffle)
        # label smoothing, mixup and CutMix of the training loss / input, keyed the same way
        self.label_smoothing, self.mixup_alpha, self.cutmix_alpha = label_smoothing, mixup_alpha, cutmix_alpha
        self.mixes = mixup_alpha > 0 or cutmix_alpha > 0
        dev = self.device = torch.device(device)
        B = batch
        self.bn_momentum = bn_momentum
        self.shortcut_even_on = os.environ.get("SL_SHORTCUT_EVEN", "1") != "0"
        # BN-on-load: where the direct 3x3 kernel serves a block's conv2 (64 channels, 32 wide), it
        # reads relu(bn1(c1)) straight from c1 -- forward and weight gradient -- and a1 is never
        # written (SL_BN_ONLOAD=0: bn_apply_stats + a1, as before)
        self.bn_onload = os.environ.get("SL_BN_ONLOAD", "1") != "0"
        n = spec.n_flat
        self.params = torch.zeros(n, dtype=torch.float32, device=dev)
        self.params.copy_((flat if flat is not None else init_params(spec, seed)).to(dev))
        self._init_state(batch, lr, momentum, weight_decay, world_size, accum_steps, opt)
        self.grad = torch.zeros_like(self.params)
        self.shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        bns = list(spec.bns())
        rsz = {b.name: (K.rsum_floats(2 * b.c) + 3) // 4 * 4 for b in bns}  # 16-B aligned regions
        self.arena = torch.zeros(sum(2 * rsz[b.name] for b in bns), device=dev)
        off = 0
        self.bn = {}
        for b in bns:
            self.bn[b.name] = _BN(b, self.params, self.grad, self.arena, off, dev, rsz[b.name])
            off += 2 * rsz[b.name]
        self.conv = {c.name: _Conv(c, self.params, self.shadow, self.grad, dev) for c in spec.convs()}
        self.fc_w = self.shadow[spec.fc_w:spec.fc_w + classes * 512]
        self.fc_b = self.params[spec.fc_b:spec.fc_b + classes]
        self.fc_gw = self.grad[spec.fc_w:spec.fc_w + classes * 512]
        self.fc_gb = self.grad[spec.fc_b:spec.fc_b + classes]
        self.fc_wt = torch.zeros(512 * self.logit_ld, dtype=torch.bfloat16, device=dev)

        bf = dict(dtype=torch.bfloat16, device=dev)
        hw = spec.in_hw
        self.x0 = torch.empty(B, hw, hw, 8, **bf)
        self.labels = torch.zeros(B, dtype=torch.uint8, device=dev)
        # (record, oy, ox, flip) of every sample of the last training batch, written by input_aug /
        # input_mix; None with the pipeline off (input_norm feeds the network, as in every
        # evaluation path)
        self.aug_out = (torch.zeros(B, 4, dtype=torch.int32, device=dev)
                        if self.shuffle or augment != "none" or self.mixes else None)
        # (partner, num, den, mode, x0, y0, x1, y1) of every sample of the last training batch, written
        # by input_mix and read by the soft-target loss; None with no mix.  mix_tab: the lambda
        # quantiles of each mode, built once (data/augment.py mix_tables)
        self.mix_out = self.mix_tab = None
        if self.mixes:
            self.mix_out = torch.zeros(B, 8, dtype=torch.int32, device=dev)
            self.mix_tab = torch.from_numpy(A.mix_tables(mixup_alpha, cutmix_alpha)).to(dev)
        # ---- stem buffers ----
        sc = spec.stem_conv
        s_hw = K.out_size(hw, sc.k, sc.stride, sc.pad)
        self.c0 = torch.empty(B, s_hw, s_hw, 64, **bf)
        self.a0 = torch.empty_like(self.c0)
        self.dc0 = torch.empty_like(self.c0)
        self.da0 = torch.empty_like(self.c0)
        cur = self.a0
        if spec.stem == "imagenet":
            p_hw = K.out_size(s_hw, 3, 2, 1)
            self.p0 = torch.empty(B, p_hw, p_hw, 64, **bf)
            self.p0_arg = torch.empty(B, p_hw, p_hw, 64, dtype=torch.uint8, device=dev)
            self.dp0 = torch.empty_like(self.p0)
            cur = self.p0
        # ---- residual blocks ----
        self.blocks = []
        for blk in spec.blocks:
            st = {"spec": blk, "x": cur}
            h = cur.shape[1]
            oh = K.out_size(h, 3, blk.conv1.stride, 1)
            shp = (B, oh, oh, blk.conv1.cout)
            for name in ("c1", "a1", "c2", "y", "dz", "dc2", "da1", "dc1"):
                st[name] = torch.empty(shp, **bf)
            # 1-bit ReLU mask of y (bit j of byte q = y[8q+j] > 0) for the backward
            st["ym"] = torch.empty(B * oh * oh * blk.conv1.cout // 8, dtype=torch.uint8, device=dev)
            if blk.down is not None:
                st["cs"] = torch.empty(shp, **bf)
                st["dcs"] = torch.empty(shp, **bf)
                if not self._shortcut_even(blk):  # else the shortcut gradient goes straight into dx
                    st["dxs"] = torch.empty_like(cur)
            st["dx"] = torch.empty_like(cur)
            c2s = blk.conv2
            st["bnin"] = self.bn_onload and K.conv3x3_bnin_applicable(shp, c2s.cout, c2s.k, c2s.stride, c2s.pad)
            self.blocks.append(st)
            cur = st["y"]
        self.feat_in = cur
        # stem BN-on-load: with an identity first block, a0 = relu(bn0(c0)) feeds only block 0's
        # conv1 (forward, weight gradient) and its residual; both rebuild it from c0
        b0 = self.blocks[0]
        c1s = b0["spec"].conv1
        self.stem_onload = (self.bn_onload and spec.stem != "imagenet" and b0["spec"].down is None
                            and K.conv3x3_bnin_applicable(self.c0.shape, c1s.cout, c1s.k, c1s.stride, c1s.pad))
        self.feat = torch.empty(B, 1, 1, 512, **bf)
        self.dfeat = torch.empty_like(self.feat)
        self.dfeat_in = torch.empty_like(cur)
        self.logits = torch.empty(B, classes, device=dev)
        self.dlogits = torch.zeros(B, 1, 1, self.logit_ld, **bf)
        # the wide loss's bias-gradient partial rows (None up to 16 classes), allocated once
        self.ce_ws = K.softmax_ce_wide_ws(B, classes, dev)
        if self.wide:
            self._ce_kw = dict(ws=self.ce_ws)
        self.loss = torch.zeros(B, device=dev)
        self.correct = torch.zeros(B, device=dev)
        self._alloc_accum()
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.x = self.y = None
        self.bucket_hook = None   # callable(flat_view) -> handle, launched during backward
        self.bucket_wait = None   # callable(handles) -> None, before the optimizer
        from ..utils.phases import PhaseProbe

        self.phases = PhaseProbe(self.device)
        self.allreduce = None     # callable(grad) -> None (simple, non-overlapped)
        self.bucket_bytes = 16 << 20
        # SL_WGRAD_SIDE=1: the slab reduces run on a side stream beside the next data gradient.  Off by
        # default: starved by the one-workgroup-per-CU conv kernels, the reduces stretched from 13 to
        # 36 us and the step got 3.6 % slower (profiles/r03_side)
        self.wgrad_side = torch.cuda.Stream(dev) if os.environ.get("SL_WGRAD_SIDE", "0") == "1" else None
        # split-K slab(s) of the weight gradients, grown on the first step
        self.wgws = K.WgradWorkspace(dev, alternate=self.wgrad_side is not None)
        # BN-backward sums in the data-gradient epilogues instead of bn_bwd_reduce passes
        self.fuse_bn_bwd = os.environ.get("SL_BNB_FUSE", "1") != "0"

        items = [(c.w, c.wt, c.spec.cout, c.spec.k * c.spec.k, c.spec.cin, c.ldt)
                 for c in self.conv.values() if c.spec.name != "stem"]
        items.append((self.fc_w, self.fc_wt, classes, 1, 512, self.logit_ld))
        self.wt = K.WeightTransposer(items, dev)
        self.refresh_shadows()
        self.stats()  # load torch's reduction kernel now, not inside the first logged chunk (as mlp.py)

    def _shortcut_even(self, blk) -> bool:
        """A 1x1 / stride-2 shortcut beside a 3x3 / stride-2 conv1 (every ResNet-18 downsample
        block): its data gradient is written straight into the (even, even) positions of the block's
        input gradient, and conv1's parity-class data gradient adds there (ops.cnn.conv_dgrad_s2_even).
        SL_SHORTCUT_EVEN=0 keeps the full-resolution shortcut gradient + add (A/B, tests)."""
        d, c1 = blk.down, blk.conv1
        return (self.shortcut_even_on and d is not None and d.k == 1 and d.stride == 2 and d.pad == 0
                and c1.k == 3 and c1.stride == 2 and c1.pad == 1 and d.cout % 64 == 0 and c1.cout % 64 == 0)

    # ------------------------------------------------------------------
    def refresh_shadows(self) -> None:
        self.O.to_bf16(self.params, self.shadow)
        self.wt()

    def load_shard(self, x_u8: torch.Tensor, y_u8: torch.Tensor) -> None:
        """The resident shard.  With the input pipeline on, the epoch is cursor // (N // batch): a
        shard of another size changes N // batch from the next step on, so the epoch index jumps."""
        hw = self.spec.in_hw
        x = x_u8.reshape(-1, hw, hw, 3)
        if x.shape[0] < self.batch:
            raise ValueError("shard smaller than one batch")
        self.x = x.to(self.device, non_blocking=True).contiguous()
        self.y = y_u8.reshape(-1).to(self.device, non_blocking=True).to(torch.uint8).contiguous()
        self.graph = None

    # ------------------------------------------------------------------
    def _conv_bn(self, x, conv: _Conv, bn: _BN, out):
        K = self.K
        c = conv.spec
        K.conv_fwd(x, conv.w, c.cout, c.k, c.stride, c.pad, y=out, stats=bn.stats_buf)

    def forward(self, train: bool = True):
        K, spec = self.K, self.spec
        self.arena.zero_()
        if train and self.mixes:
            K.input_mix(self.x, self.y, self.cursor, self.batch, self.x0, self.labels, self.aug_out, self.mix_out,
                        self.mix_tab, CIFAR_MEAN, CIFAR_STD, seed=self.seed, shuffle=self.shuffle,
                        augment=self.augment, pad=self.augment_pad, mixup=self.mixup_alpha > 0,
                        cutmix=self.cutmix_alpha > 0)
        elif train and self.aug_out is not None:
            K.input_aug(self.x, self.y, self.cursor, self.batch, self.x0, self.labels, self.aug_out, CIFAR_MEAN,
                        CIFAR_STD, seed=self.seed, shuffle=self.shuffle, augment=self.augment,
                        pad=self.augment_pad)
        else:
            K.input_norm(self.x, self.y, self.cursor, self.batch, self.x0, self.labels, CIFAR_MEAN, CIFAR_STD)
        sbn = self.bn[spec.stem_bn.name]
        self._conv_bn(self.x0, self.conv["stem"], sbn, self.c0)
        cnt0 = self.c0.numel() // 64
        if not self.stem_onload:
            K.bn_apply_stats(self.c0, sbn, self.a0, cnt0, momentum=self.bn_momentum)
        if spec.stem == "imagenet":
            K.maxpool_fwd(self.a0, self.p0, self.p0_arg)
        for i, st in enumerate(self.blocks):
            blk: BlockSpec = st["spec"]
            b1, b2 = self.bn[blk.bn1.name], self.bn[blk.bn2.name]
            stem_in = i == 0 and self.stem_onload
            if stem_in:
                K.conv3x3_bnin_fwd(self.c0, self.conv[blk.conv1.name].w, sbn, cnt0, st["c1"], stats=b1.stats_buf,
                                   momentum=self.bn_momentum)
            else:
                self._conv_bn(st["x"], self.conv[blk.conv1.name], b1, st["c1"])
            cnt = st["c1"].numel() // blk.conv1.cout
            if st["bnin"]:
                K.conv3x3_bnin_fwd(st["c1"], self.conv[blk.conv2.name].w, b1, cnt, st["c2"], stats=b2.stats_buf,
                                   momentum=self.bn_momentum)
            else:
                K.bn_apply_stats(st["c1"], b1, st["a1"], cnt, momentum=self.bn_momentum)
                self._conv_bn(st["a1"], self.conv[blk.conv2.name], b2, st["c2"])
            if blk.down is not None:
                bd = self.bn[blk.dbn.name]
                self._conv_bn(st["x"], self.conv[blk.down.name], bd, st["cs"])
                K.bn_apply_stats(st["c2"], b2, st["y"], cnt, res=st["cs"], rbn=bd, momentum=self.bn_momentum,
                                 mask_out=st["ym"])
            elif stem_in:
                K.bn_apply_stats(st["c2"], b2, st["y"], cnt, res=self.c0, rbn=sbn, res_relu=True,
                                 momentum=self.bn_momentum, mask_out=st["ym"])
            else:
                K.bn_apply_stats(st["c2"], b2, st["y"], cnt, res=st["x"], momentum=self.bn_momentum,
                                 mask_out=st["ym"])
        K.avgpool_fwd(self.feat_in, self.feat)
        K.conv_fwd(self.feat, self.fc_w, spec.classes, 1, 1, 0, yf=self.logits, bias=self.fc_b)
        if train and (self.mixes or self.label_smoothing > 0):
            # soft targets; `correct` stays the argmax against the sample's own label (a diagnostic
            # under mixing)
            K.softmax_ce_soft(self.logits, self.labels, self.loss, self.correct,
                              self.dlogits.view(self.batch, self.logit_ld), self.fc_gb, self.grad_scale,
                              mix=self.mix_out, eps=self.label_smoothing, **self._ce_kw)
        else:
            K.softmax_ce(self.logits, self.labels, self.loss, self.correct,
                         self.dlogits.view(self.batch, self.logit_ld), self.fc_gb if train else None,
                         self.grad_scale, **self._ce_kw)

    def backward(self, hook: bool = True, fold: bool = False):
        """``hook=False``: no bucket hook is called (an accumulated step's earlier micro-batches).
        ``fold``: the partial sum ``acc`` of the earlier micro-batches is added into each bucket's
        range of ``grad`` just before the hook takes it (the last micro-batch)."""
        K, spec = self.K, self.spec
        handles = []
        pending_from = spec.n_flat  # grad[pending_from:] is final and not yet reduced
        bucket_elems = self.bucket_bytes // 4

        side = self.wgrad_side
        if side is not None:
            K.wgrad_side_begin(side)

        def maybe_bucket(lo, force=False):
            nonlocal pending_from
            if self.bucket_hook is None or not hook:
                return
            if force or (pending_from - lo) >= bucket_elems:
                if side is not None:
                    K.wgrad_side_join(end=False)  # the bucket's reduces are in the gradient
                if fold:
                    self.O.accum_flat(self.grad[lo:pending_from], self.acc[lo:pending_from], True)
                handles.append(self.bucket_hook(self.grad[lo:pending_from]))
                pending_from = lo

        K.conv_wgrad(self.feat, self.dlogits, spec.classes, 1, 1, 0, self.fc_gw, ws=self.wgws)
        K.conv_dgrad(self.dlogits, self.fc_wt, 512, 1, 1, 0, self.dfeat)
        K.avgpool_bwd(self.dfeat.view(self.batch, 512), self.dfeat_in)
        dy = self.dfeat_in
        fuse = self.fuse_bn_bwd
        sbn = self.bn[spec.stem_bn.name]
        rblocks = list(reversed(self.blocks))

        def block_out_bn(st):
            # BN backward of a block output y = relu(bn2(c2) + sc): the mask is the forward's
            # 1-bit image of y; a downsample shortcut's BN (input cs) is fed by the same dz
            blk = st["spec"]
            b2 = self.bn[blk.bn2.name]
            d = dict(x=st["c2"], sums=b2.sums_buf, y_mask=st["ym"])
            if blk.down is not None:
                d.update(x2=st["cs"], sums2=self.bn[blk.dbn.name].sums_buf)
            return d

        for i, st in enumerate(rblocks):
            blk: BlockSpec = st["spec"]
            c1, c2 = self.conv[blk.conv1.name], self.conv[blk.conv2.name]
            b1, b2 = self.bn[blk.bn1.name], self.bn[blk.bn2.name]
            # y = relu(bn2(c2) + sc): dz = dy * 1[y > 0] feeds bn2 and the shortcut.  Fused: the
            # previous conv1 data gradient (next block's) already stored dz and the sums.
            down = blk.down is not None
            bd = self.bn[blk.dbn.name] if down else None
            if not (fuse and i > 0):
                bo = block_out_bn(st)
                K.bn_bwd_reduce(dy, None, bo["x"], bo["sums"], dz_out=st["dz"], y_mask=bo["y_mask"],
                                x2=bo.get("x2"), sums2=bo.get("sums2"))
            # the input gradient is the previous block's output gradient (its dz, stored masked
            # with that block's BN sums) or, for the first block, the stem BN's
            nxt = None
            if fuse and i + 1 < len(rblocks):
                nxt = block_out_bn(rblocks[i + 1])
                dx = rblocks[i + 1]["dz"]
            elif fuse and spec.stem != "imagenet":
                nxt = dict(x=self.c0, sums=sbn.sums_buf, mask_coef=sbn.coef)
                dx = st["dx"]
            else:
                dx = st["dx"]
            add, add_even = st["dz"], False
            if down:
                cd = self.conv[blk.down.name]
                # dc2 and dcs from one read of dz
                K.bn_bwd_apply_dual(st["dz"], st["c2"], b2.sums, b2.coef, b2.ggamma, b2.gbeta, st["dc2"],
                                    st["cs"], bd.sums, bd.coef, bd.ggamma, bd.gbeta, st["dcs"])
                K.conv_wgrad(st["x"], st["dcs"], blk.down.cout, 1, blk.down.stride, 0, cd.g, ws=self.wgws)
                if self._shortcut_even(blk):
                    # 1x1/s2 shortcut: only the (even, even) positions of dx get a gradient; write
                    # them into dx now, and conv1's parity-class data gradient adds there
                    K.conv_dgrad_s2_even(st["dcs"], cd.wt, blk.down.cin, dx)
                    add, add_even = dx, True
                else:
                    K.conv_dgrad(st["dcs"], cd.wt, blk.down.cin, 1, blk.down.stride, 0, st["dxs"])
                    add = st["dxs"]
            else:
                K.bn_bwd_apply_sums(st["dz"], None, st["c2"], b2.sums, b2.coef, b2.ggamma, b2.gbeta, st["dc2"])
            if st["bnin"]:
                K.conv3x3_bnin_wgrad(st["c1"], st["dc2"], b1, st["c1"].numel() // blk.conv1.cout, c2.g, ws=self.wgws)
            else:
                K.conv_wgrad(st["a1"], st["dc2"], blk.conv2.cout, 3, 1, 1, c2.g, ws=self.wgws)
            # a1 = relu(bn1(c1)): the mask is re-derived from c1 and bn1's coefficients
            bn1 = dict(x=st["c1"], sums=b1.sums_buf, mask_coef=b1.coef)
            if fuse:
                K.conv_dgrad(st["dc2"], c2.wt, blk.conv2.cin, 3, 1, 1, st["da1"], bn=bn1)
            else:
                K.conv_dgrad(st["dc2"], c2.wt, blk.conv2.cin, 3, 1, 1, st["da1"])
                K.bn_bwd_reduce(st["da1"], None, st["c1"], b1.sums_buf, mask_coef=b1.coef)
            K.bn_bwd_apply_sums(st["da1"], None, st["c1"], b1.sums, b1.coef, b1.ggamma, b1.gbeta, st["dc1"],
                                mask_coef=b1.coef)
            if st is self.blocks[0] and self.stem_onload:
                K.conv3x3_bnin_wgrad(self.c0, st["dc1"], sbn, self.c0.numel() // 64, c1.g, ws=self.wgws)
            else:
                K.conv_wgrad(st["x"], st["dc1"], blk.conv1.cout, 3, blk.conv1.stride, 1, c1.g, ws=self.wgws)
            K.conv_dgrad(st["dc1"], c1.wt, blk.conv1.cin, 3, blk.conv1.stride, 1, dx, add=add, bn=nxt,
                         add_even=add_even)
            dy = dx
            maybe_bucket(blk.conv1.off)
        # stem
        if spec.stem == "imagenet":
            K.maxpool_bwd(dy, self.p0_arg, self.da0)
            dy = self.da0
        if not (fuse and spec.stem != "imagenet"):
            K.bn_bwd_reduce(dy, None, self.c0, sbn.sums_buf, mask_coef=sbn.coef)
        K.bn_bwd_apply_sums(dy, None, self.c0, sbn.sums, sbn.coef, sbn.ggamma, sbn.gbeta, self.dc0,
                            mask_coef=sbn.coef)
        sc = spec.stem_conv
        K.conv_wgrad(self.x0, self.dc0, 64, sc.k, sc.stride, sc.pad, self.conv["stem"].g, ws=self.wgws)
        maybe_bucket(0, force=True)
        if side is not None:
            K.wgrad_side_join(end=True)
        return handles

    def _accum_sums(self, i: int) -> None:
        """After micro-batch ``i`` of an accumulated step: its gradient, per-sample loss and correct
        into the partial sums (stored after the first, added after the others)."""
        for a, t in ((self.acc, self.grad), (self.loss_acc, self.loss), (self.correct_acc, self.correct)):
            self.O.accum_flat(a, t, i > 0)

    def _step_eager(self) -> None:
        self.grad.zero_()
        if not torch.cuda.is_current_stream_capturing():
            self.wgws.grow()  # size the split-K slab before any capture (first call: atomics)
        last = self.accum_steps - 1
        for i in range(last):  # an accumulated step's earlier micro-batches: no exchange
            self.forward(train=True)
            self.backward(hook=False)
            self._accum_sums(i)
            self.K.cursor_bump(self.cursor)
            self.grad.zero_()
        self.forward(train=True)
        # grad = ((g_0 + g_1) + ...) + g_last: bucket by bucket ahead of each hook, so the bucket
        # all-reduces still overlap the rest of this backward; in one launch with no bucket hook
        handles = self.backward(fold=last > 0)
        if last > 0:
            if self.bucket_hook is None:
                self.O.accum_flat(self.grad, self.acc, True)
            self.O.accum_flat(self.loss, self.loss_acc, True)
            self.O.accum_flat(self.correct, self.correct_acc, True)
        self.phases.mark("compute")
        if self.bucket_wait is not None:
            self.bucket_wait(handles)  # the bucket all-reduces ran during backward: the exposed part
        if self.allreduce is not None:
            self.allreduce(self.grad)
        self.phases.mark("exchange")
        if self.opt.clips:  # on the aggregated gradient, before the unchanged update rule
            self.O.clip_grad_norm_flat(self.grad, self.opt.clip_grad_norm, self.clip_partials, self.clip_norm)
        self._update()
        if self.ema is not None:  # on the parameters just written; the launch advances ema_step itself
            self.O.ema_flat(self.ema, self.params, self.ema_step, self.ema_ticket, self.ema_tab)
        self.wt()
        self.K.cursor_bump(self.cursor)
        self.phases.mark("update")

    def _update(self) -> None:
        """The optimizer launch (the step-counter rules: plus the bump of the optimizer step)."""
        O = self.O
        if self.opt_step is None:
            O.sgd_flat(self.params, self.grad, self.mom, self.lr, self.momentum, self.weight_decay,
                       shadow=self.shadow)
            return
        if self.opt.grouped:  # a weight decay per class (BatchNorm, fc.bias), read from the map
            if self.opt.adamw:
                O.adamw_flat_groups(self.params, self.grad, self.mom, self.v, self.opt_step, self.opt, self.decay_cls,
                                    self.lr_tab, shadow=self.shadow)
            else:
                O.sgd_flat_lr_groups(self.params, self.grad, self.mom, self.opt_step, self.lr_tab, self.decay_cls,
                                     self.opt.decays(), lr=self.lr, momentum=self.momentum, shadow=self.shadow)
        elif self.opt.adamw:
            O.adamw_flat(self.params, self.grad, self.mom, self.v, self.opt_step, self.opt, self.lr_tab,
                         shadow=self.shadow)
        else:
            O.sgd_flat_lr(self.params, self.grad, self.mom, self.opt_step, self.lr_tab, self.momentum,
                          self.weight_decay, shadow=self.shadow)
        self.K.cursor_bump(self.opt_step)

    def probe_step(self):
        """One eager training step with its phase boundaries recorded (utils/phases.py): returns
        a PendingPhases, resolved by the caller once the device has finished the step."""
        self.phases.arm()
        self._step_eager()
        pending = self.phases.finish()
        hooked = self.allreduce is not None or self.bucket_hook is not None
        pending.exchange_bytes = 4 * int(self.grad.numel()) if hooked else 0
        return pending

    # ------------------------------------------------------------------
    def compute_grads(self) -> torch.Tensor:
        """Forward + backward on the current batch (no update, no cursor bump)."""
        self.grad.zero_()
        self.forward(train=True)
        self.backward()
        return self.grad

    def stats(self) -> StepStats:
        n = self.samples_per_step  # (an accumulated step leaves the sums over its micro-batches in loss / correct)
        return StepStats(float(self.loss.sum()) / n, float(self.correct.sum()) / n, n)

    def get_flat(self) -> torch.Tensor:
        return self.params.clone()

    def set_flat(self, flat: torch.Tensor) -> None:
        self.params.copy_(flat.to(self.params))
        self.refresh_shadows()

    def running_stats(self) -> dict:
        return {name: (b.run_mean, b.run_var) for name, b in self.bn.items()}

    # ---- inference with running statistics ----
    def _eval_coef(self, bn: _BN, eps: float = 1e-5) -> torch.Tensor:
        sc = bn.gamma * torch.rsqrt(bn.run_var + eps)
        return torch.cat([sc, bn.beta - bn.run_mean * sc, bn.run_mean, torch.rsqrt(bn.run_var + eps)])

    def forward_eval(self) -> None:
        """Eval-mode forward of the current batch: every BatchNorm normalises with its running
        statistics (no batch statistics are computed, none are updated), then loss / correct
        / logits.  Same kernels as training -- conv_fwd without the statistics epilogue and
        bn_apply with coefficients folded from (gamma, beta, running mean, running var)."""
        K, spec = self.K, self.spec
        co = {name: self._eval_coef(b) for name, b in self.bn.items()}
        K.input_norm(self.x, self.y, self.cursor, self.batch, self.x0, self.labels, CIFAR_MEAN, CIFAR_STD)
        sc = spec.stem_conv
        K.conv_fwd(self.x0, self.conv["stem"].w, sc.cout, sc.k, sc.stride, sc.pad, y=self.c0)
        K.bn_apply(self.c0, co[spec.stem_bn.name], self.a0, relu=True)
        if spec.stem == "imagenet":
            K.maxpool_fwd(self.a0, self.p0, self.p0_arg)
        for st in self.blocks:
            blk: BlockSpec = st["spec"]
            c1, c2 = blk.conv1, blk.conv2
            K.conv_fwd(st["x"], self.conv[c1.name].w, c1.cout, c1.k, c1.stride, c1.pad, y=st["c1"])
            K.bn_apply(st["c1"], co[blk.bn1.name], st["a1"], relu=True)
            K.conv_fwd(st["a1"], self.conv[c2.name].w, c2.cout, c2.k, c2.stride, c2.pad, y=st["c2"])
            if blk.down is not None:
                d = blk.down
                K.conv_fwd(st["x"], self.conv[d.name].w, d.cout, d.k, d.stride, d.pad, y=st["cs"])
                K.bn_apply(st["c2"], co[blk.bn2.name], st["y"], relu=True, res=st["cs"], rcoef=co[blk.dbn.name])
            else:
                K.bn_apply(st["c2"], co[blk.bn2.name], st["y"], relu=True, res=st["x"])
        K.avgpool_fwd(self.feat_in, self.feat)
        K.conv_fwd(self.feat, self.fc_w, spec.classes, 1, 1, 0, yf=self.logits, bias=self.fc_b)
        K.softmax_ce(self.logits, self.labels, self.loss, self.correct, self.dlogits.view(self.batch, self.logit_ld),
                     None, self.grad_scale, **self._ce_kw)

    @contextlib.contextmanager
    def _ema_weights(self):
        """``ema=True`` of the evaluations: the parameters' contents become the average's and are put
        back (with the bf16 shadow; the transposed weights are rebuilt from it).  No tensor moves, so
        a captured graph stays valid."""
        if self.ema is None:
            raise ValueError("evaluate(ema=True): this trainer keeps no weight EMA (ema_decay=0)")
        keep = (self.params.clone(), self.shadow.clone())
        self.params.copy_(self.ema)
        self.refresh_shadows()
        try:
            yield
        finally:
            self.params.copy_(keep[0])
            self.shadow.copy_(keep[1])
            self.wt()

    @contextlib.contextmanager
    def _eval_shard(self, x: torch.Tensor, y: torch.Tensor):
        """(x, y) on the device as the current shard, read from batch 0 on by a cursor of its own; the
        training shard and cursor are put back untouched."""
        saved = (self.x, self.y, self.cursor)
        self.x, self.y, self.cursor = x, y, torch.zeros(1, dtype=torch.int32, device=self.device)
        try:
            yield
        finally:
            self.x, self.y, self.cursor = saved

    def evaluate(self, x_u8: torch.Tensor, y_u8: torch.Tensor, ema: bool = False) -> StepStats:
        """Eval-mode loss / accuracy over every whole batch of (x, y) with the running
        statistics; the training shard, cursor and statistics are left untouched.  ``ema=True``:
        of the averaged parameters, with the same running statistics -- what a second trainer
        returns after ``set_flat(ema_flat())`` (:meth:`_ema_weights`).  Between steps only."""
        if ema:
            with self._ema_weights():
                return self.evaluate(x_u8, y_u8)
        hw = self.spec.in_hw
        x = x_u8.reshape(-1, hw, hw, 3).to(self.device).contiguous()
        y = y_u8.reshape(-1).to(self.device).to(torch.uint8).contiguous()
        nb = x.shape[0] // self.batch
        if nb < 1:
            raise ValueError("evaluation set smaller than one batch")
        loss = corr = 0.0
        with self._eval_shard(x, y):
            for _ in range(nb):
                self.forward_eval()
                loss += float(self.loss.sum())
                corr += float(self.correct.sum())
                self.K.cursor_bump(self.cursor)
        n = nb * self.batch
        return StepStats(loss / n, corr / n, n)

    # ---- the held-out evaluation pass (ops/evalmetrics.py) ----
    def _eval_padded(self, x_u8: torch.Tensor, y_u8: torch.Tensor) -> tuple:
        """(x, y, N) on the device, zero-padded to whole batches; cached by the identity of the
        tensors passed (and kept with them), so a worker's repeated evaluations copy once."""
        c = self._eval_cache
        if c is not None and c[0] is x_u8 and c[1] is y_u8:
            return c[2], c[3], c[4]
        hw = self.spec.in_hw
        y = y_u8.reshape(-1)
        N = self.E.check_records(int(y.numel()))
        x = x_u8.reshape(N, hw, hw, 3)
        rows = (N + self.batch - 1) // self.batch * self.batch
        xp = torch.zeros(rows, hw, hw, 3, dtype=torch.uint8, device=self.device)
        yp = torch.zeros(rows, dtype=torch.uint8, device=self.device)
        xp[:N].copy_(x)
        yp[:N].copy_(y)
        self._eval_cache = (x_u8, y_u8, xp, yp, N)
        return xp, yp, N

    def evaluate_full(self, x_u8: torch.Tensor, y_u8: torch.Tensor, ema: bool = False, topk: int = 5):
        """The held-out report (EvalReport) over EVERY record of (x, y), running statistics as in
        :meth:`evaluate`.  The set is padded with zero records to whole batches; per batch one
        ``forward_eval``, one ``sl_eval_accum`` launch that counts the batch's first ``n_valid`` rows into
        an integer block on the device (264 words up to 16 classes, 8 + classes^2 above), and the cursor bump.  The host waits once, for the block
        after the last batch: nothing in the loop reads the device.  Eval-mode BatchNorm normalises each
        row with the running statistics, so the padding rows cannot reach the valid ones.  ``ema=True``
        as in :meth:`evaluate`; training state, cursor and running statistics are bit-identical
        afterwards and no tensor moves, so a captured graph stays valid.  Between steps only."""
        E = self.E
        topk = E.check_topk(topk, self.spec.classes)
        if ema:
            with self._ema_weights():
                return self.evaluate_full(x_u8, y_u8, topk=topk)
        x, y, N = self._eval_padded(x_u8, y_u8)
        B = self.batch
        ncls = self.spec.classes
        # more than 16 classes: eval_accum_wide_kernel and its 8 + ncls^2 word block
        accum, from_acc = (E.eval_accum_wide, E.report_from_acc_wide) if self.wide else (E.eval_accum, E.report_from_acc)
        acc = E.new_acc_wide(self.device, ncls) if self.wide else E.new_acc(self.device)
        with self._eval_shard(x, y):
            for b in range(x.shape[0] // B):
                self.forward_eval()
                accum(self.logits, self.labels, self.loss, min(B, N - b * B), ncls, topk, acc)
                self.K.cursor_bump(self.cursor)
        return from_acc(acc, ncls, topk)
