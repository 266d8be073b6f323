"""ctypes bindings of the CNN kernels (csrc/kernels/conv.hip, cnn_aux.hip).

Thin, shape-checked wrappers: every function takes torch tensors (NHWC bf16
activations, fp32 statistics/gradients) and launches on the current stream,
so the CNN engine's whole step can be captured in a hipGraph.  No fallback:
on a GPU box a missing or failing kernel raises.
"""
from __future__ import annotations

import ctypes

import os

import torch

from . import _native as N

# bit i of sl_conv_kernels_seen = family i (csrc/kernels/common.h SlConvFamily, same order)
KERNEL_FAMILIES = (
    "gemm_64x64", "gemm_64x128", "gemm_128x64", "gemm_128x128",
    "gemm_t_64x64", "gemm_t_64x128", "gemm_t_128x64", "gemm_t_128x128",
    "big", "big_t", "wide", "wide_t", "wide128", "wide128_t",
    "dgrad_s2", "dgrad_s2_alt",
    "wgrad_64", "wgrad_64_lean", "wgrad_128", "wgrad_128_lean", "wgrad_big", "wgrad_big_lean",
    "halo_fwd_c64", "halo_fwd_c8", "halo_dgrad", "halo_wgrad",
)


def conv_kernels_seen(clear: bool = False) -> frozenset:
    """Names (:data:`KERNEL_FAMILIES`) of the convolution kernel families launched since the last
    clear -- a host-side record kept by the launchers, so a test can assert which kernel a shape
    reached.  ``clear`` resets the record after reading it."""
    mask = int(N.lib().sl_conv_kernels_seen(1 if clear else 0))
    assert mask >> len(KERNEL_FAMILIES) == 0, hex(mask)
    return frozenset(name for i, name in enumerate(KERNEL_FAMILIES) if mask >> i & 1)

p = N.ptr


def _bf16(t):
    assert t.dtype == torch.bfloat16 and t.is_contiguous(), (t.dtype, t.shape)
    return p(t)


def _f32(t):
    if t is None:
        return None
    assert t.dtype == torch.float32 and t.is_contiguous()
    return p(t)


def rsum_floats(n: int) -> int:
    """Size of a cross-workgroup sum buffer for n values (replicas | result | pad)."""
    return int(N.lib().sl_rsum_floats(n))


def rsum_result(buf: torch.Tensor, n: int) -> torch.Tensor:
    """The folded result (n floats) inside an rsum buffer."""
    off = int(N.lib().sl_rsum_result_offset(n))
    return buf[off:off + n]


def out_size(h: int, k: int, s: int, pad: int) -> int:
    return (h + 2 * pad - k) // s + 1


def conv_fwd(x, w, cout: int, k: int, stride: int, pad: int, y=None, yf=None, bias=None, stats=None, ldy=None):
    """x [N,H,W,C] bf16, w [cout, k*k*C] bf16 -> y [N,OH,OW,ldy] bf16 and/or yf [N*OH*OW, cout] fp32."""
    n, h, wd, c = x.shape
    oh, ow = out_size(h, k, stride, pad), out_size(wd, k, stride, pad)
    assert w.numel() >= cout * k * k * c
    if y is not None:
        assert y.shape[:3] == (n, oh, ow), (y.shape, n, oh, ow)
        ldy = y.shape[3]
    N.call("sl_conv_fwd", _bf16(x), n, h, wd, c, _bf16(w), cout, k, k, stride, pad, oh, ow,
           _bf16(y) if y is not None else None, int(ldy or cout), _f32(yf), _f32(bias), _f32(stats), N.stream_ptr())
    return oh, ow


def conv_dgrad_s2_even(dy, wt, cin: int, dx):
    """Data gradient of a 1x1 / stride-2 / pad-0 convolution written to the (even, even) positions of
    dx [N,H,W,cin] only; the other positions are left as they are.  A downsample block passes dx
    on as ``add`` with ``add_even=True`` to its strided 3x3 conv1 data gradient, which writes every
    position and adds the shortcut's part at the even ones (csrc/kernels/conv.hip)."""
    n, oh, ow, cd = dy.shape
    _, h, wd, ci = dx.shape
    assert ci == cin and (h + 1) // 2 == oh and (wd + 1) // 2 == ow
    N.call("sl_conv_dgrad_s2_even", _bf16(dy), n, oh, ow, cd, _bf16(wt), cin, h, wd, _bf16(dx), N.stream_ptr())


def conv_dgrad(dy, wt, cin: int, k: int, stride: int, pad: int, dx, add=None, bn=None, add_even: bool = False):
    """dy [N,OH,OW,Cd] bf16 (Cd channels, zero beyond cout), wt [cin, k*k*Cd] -> dx [N,H,W,cin] (+ add).

    ``add_even`` (3x3 stride-2 only): ``add`` holds values at the (even, even) positions only and
    may be dx itself (see :func:`conv_dgrad_s2_even`).

    ``bn``: dx is the gradient at the input of ``relu(bn(x))`` (or of a block output
    ``relu(bn(x) + shortcut)``): a dict with ``x`` (the BN input, dx's shape), ``sums``
    (its zeroed rsum buffer) and the ReLU mask as ``mask_coef`` or ``y_mask`` -- the keys
    of :func:`bn_bwd_reduce`, optionally with ``x2``/``sums2``.  dx is then stored masked
    and the BN-backward sums are accumulated by the conv epilogue, replacing a
    :func:`bn_bwd_reduce` pass (csrc/kernels/bn_bwd_epi.h)."""
    n, oh, ow, cd = dy.shape
    _, h, wd, ci = dx.shape
    assert ci == cin
    if add is not None:
        assert add.shape == dx.shape and add.dtype == torch.bfloat16
    assert not add_even or (add is not None and k == 3 and stride == 2 and pad == 1)
    if bn is None:
        if add_even:
            N.call("sl_conv_dgrad_bnx", _bf16(dy), n, oh, ow, cd, _bf16(wt), cin, k, k, stride, pad, h, wd,
                   _bf16(dx), _bf16(add), None, None, None, None, None, None, 1, N.stream_ptr())
            return
        N.call("sl_conv_dgrad", _bf16(dy), n, oh, ow, cd, _bf16(wt), cin, k, k, stride, pad, h, wd, _bf16(dx),
               _bf16(add) if add is not None else None, N.stream_ptr())
        return
    x, ym, mc, x2 = bn["x"], bn.get("y_mask"), bn.get("mask_coef"), bn.get("x2")
    assert x.shape == dx.shape and dx.is_contiguous() and (ym is None or mc is None)
    if ym is not None:
        assert ym.dtype == torch.uint8 and ym.numel() * 8 == x.numel() and ym.is_contiguous()
    assert (x2 is None) == (bn.get("sums2") is None) and (x2 is None or x2.shape == x.shape)
    N.call("sl_conv_dgrad_bnx", _bf16(dy), n, oh, ow, cd, _bf16(wt), cin, k, k, stride, pad, h, wd, _bf16(dx),
           _bf16(add) if add is not None else None, _bf16(x), p(ym) if ym is not None else None,
           _f32(mc) if mc is not None else None, _f32(bn["sums"]), _bf16(x2) if x2 is not None else None,
           _f32(bn["sums2"]) if x2 is not None else None, 1 if add_even else 0, N.stream_ptr())


# split-K target for the implicit-GEMM weight gradient (workgroups per launch);
# SL_WGRAD_WGS overrides it for A/B runs
_WGRAD_WGS = int(os.environ.get("SL_WGRAD_WGS", "384"))  # re-swept on round-5 kernels: profiles/r05_sweep


NEED_WS = 7  # csrc/kernels/common.h SL_NEED_WS


def deterministic() -> bool:
    """True when the loaded kernel library is the deterministic build (fixed-point
    cross-workgroup sums, no split-K atomics: bit-identical runs)."""
    fn = getattr(N.lib(), "sl_deterministic", None)
    return bool(fn and fn())


class WgradWorkspace:
    """Slab for the weight gradient's split-K partials (plain stores + one ordered reduce
    launch instead of fp32 atomics into dw).  Sized by the launcher's own request: a call
    that finds it too small falls back to atomics and records the size it wanted, and
    :meth:`grow` (outside graph capture) makes the next call fit.  ``alternate``: two slabs
    handed out in turn (:meth:`take`), so a reduce running on a side stream
    (:func:`wgrad_side_begin`) does not block the next weight gradient's slab."""

    def __init__(self, device, floats: int = 0, alternate: bool = False):
        self.device = torch.device(device)
        self.bufs = [torch.empty(max(4, floats), dtype=torch.float32, device=device)
                     for _ in range(2 if alternate else 1)]
        self.i = 0

    @property
    def buf(self):
        return self.bufs[self.i]

    def take(self):
        b = self.bufs[self.i]
        self.i = (self.i + 1) % len(self.bufs)
        return b

    def untake(self) -> None:
        """Hand the slab of the last :meth:`take` out again (a call retried after :meth:`grow`
        keeps the alternation parity it would have had)."""
        self.i = (self.i - 1) % len(self.bufs)

    def grow(self) -> bool:
        need = int(N.lib().sl_conv_wgrad_ws_need())
        if need > self.bufs[0].numel():
            # a side-stream reduce (wgrad_side_begin) may still read the old slabs: let every
            # queued use finish before the caching allocator may hand their memory out again
            # (grow runs eagerly, outside graph capture, and rarely)
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            self.bufs = [torch.empty(need, dtype=torch.float32, device=self.device) for _ in self.bufs]
            return True
        return False


def wgrad_side_begin(side_stream) -> None:
    """Route the slab reduces of the following weight gradients to ``side_stream`` (forked from
    the current stream per reduce, so it works inside a hipGraph capture); end with
    :func:`wgrad_side_join`."""
    N.call("sl_wgrad_side_begin", ctypes.c_void_p(side_stream.cuda_stream))


def wgrad_side_join(end: bool = True) -> None:
    """The current stream waits for every reduce issued so far; ``end`` stops the routing."""
    N.call("sl_wgrad_side_join", N.stream_ptr(), 1 if end else 0)


def conv_wgrad(x, dy, cout: int, k: int, stride: int, pad: int, dw, target_wgs: int = 0, ws=None):
    """dw [cout, k*k*C] fp32 += sum over pixels dy^T im2col(x).  ``ws``: WgradWorkspace."""
    n, h, wd, c = x.shape
    _, oh, ow, ldy = dy.shape
    assert dw.dtype == torch.float32 and dw.numel() >= cout * k * k * c
    for attempt in range(2):
        buf = ws.take() if ws is not None else None
        rc = N.lib().sl_conv_wgrad(_bf16(x), n, h, wd, c, _bf16(dy), ldy, cout, k, k, stride, pad, oh, ow, p(dw),
                                   int(target_wgs or _WGRAD_WGS), p(buf), int(buf.numel()) if buf is not None else 0,
                                   N.stream_ptr())
        # deterministic kernel build: no atomic split-K fallback, the workspace must fit (grown
        # here, eagerly: a first step runs before any graph capture)
        if rc == NEED_WS and ws is not None and attempt == 0 and not torch.cuda.is_current_stream_capturing():
            ws.grow()
            ws.untake()
            continue
        if rc != 0:
            raise RuntimeError(f"sl_conv_wgrad failed with code {rc}")
        return


def conv3x3_bnin_applicable(x_shape, cout: int, k: int, stride: int, pad: int) -> bool:
    """Whether :func:`conv3x3_bnin_fwd` / :func:`conv3x3_bnin_wgrad` serve this convolution of a
    BN output: the direct 3x3 kernel's 64 -> 64 / stride-1 / 32-wide case (csrc/kernels/conv3x3_halo.hip)."""
    n, h, w, c = x_shape
    return (c == 64 and cout == 64 and k == 3 and stride == 1 and pad == 1
            and bool(N.lib().sl_conv3x3_c64_applicable(h, w, c, cout, 3, 3, 1, 1, c)))


def conv3x3_bnin_fwd(x, w, bn, count: int, y, stats=None, eps: float = 1e-5, momentum: float = 0.1):
    """y = conv3x3(relu(bn(x))) with the BatchNorm applied to each input chunk between its load and
    the LDS store: bn_apply_stats's output is never written or read back.  ``bn`` exposes stats
    (folded sums), gamma, beta, coef, run_mean, run_var; the kernel publishes coef and the running
    statistics as :func:`bn_apply_stats` would.  ``stats``: the output BN's rsum buffer (folded here)."""
    n, h, wd, c = x.shape
    assert y.shape[:3] == (n, h, wd) and y.is_contiguous()
    N.call("sl_conv3x3_bnin_fwd", _bf16(x), _bf16(w), n, h, _bf16(y), int(y.shape[3]), _f32(stats), _f32(bn.stats),
           _f32(bn.gamma), _f32(bn.beta), _f32(bn.coef), _f32(bn.run_mean), _f32(bn.run_var), float(count),
           float(eps), float(momentum), N.stream_ptr())


def conv3x3_bnin_wgrad(x, dy, bn, count: int, dw, ws=None, eps: float = 1e-5):
    """dw += weight gradient of the convolution fed by :func:`conv3x3_bnin_fwd`: the operand
    relu(bn(x)) is rebuilt on load from the BN input ``x`` (same bf16 values as the forward)."""
    n, h, wd, c = x.shape
    assert dy.shape == (n, h, wd, 64) and dw.dtype == torch.float32 and dw.numel() >= 64 * 9 * 64
    for attempt in range(2):
        buf = ws.take() if ws is not None else None
        rc = N.lib().sl_conv3x3_bnin_wgrad(_bf16(x), _bf16(dy), n, h, p(dw), p(buf),
                                           int(buf.numel()) if buf is not None else 0, _f32(bn.stats),
                                           _f32(bn.gamma), _f32(bn.beta), float(count), float(eps), N.stream_ptr())
        if rc == NEED_WS and ws is not None and attempt == 0 and not torch.cuda.is_current_stream_capturing():
            ws.grow()
            ws.untake()
            continue
        if rc != 0:
            raise RuntimeError(f"sl_conv3x3_bnin_wgrad failed with code {rc}")
        return


class WtDesc(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p), ("wt", ctypes.c_void_p), ("cout", ctypes.c_int), ("taps", ctypes.c_int),
                ("cin", ctypes.c_int), ("ldt", ctypes.c_int), ("begin", ctypes.c_long)]


class WeightTransposer:
    """Multi-tensor Wt[ci][tap][co] = W[co][tap][ci] for every conv (one launch)."""

    def __init__(self, items, device):
        """items: [(w_bf16_view, wt_bf16_view, cout, taps, cin, ldt)]"""
        assert ctypes.sizeof(WtDesc) == N.lib().sl_conv_wt_desc_size()
        arr = (WtDesc * len(items))()
        total = 0
        for i, (w, wt, cout, taps, cin, ldt) in enumerate(items):
            assert wt.numel() == cin * taps * ldt and w.numel() >= cout * taps * cin
            arr[i] = WtDesc(p(w), p(wt), cout, taps, cin, ldt, total)
            total += taps * ((ldt + 63) // 64) * ((cin + 63) // 64)  # 64x64 tiles
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.desc = host.to(device)
        self.n = len(items)
        self.total = total

    def __call__(self):
        N.call("sl_conv_wt", p(self.desc), self.n, self.total, N.stream_ptr())


def input_norm(x_u8, labels, cursor, batch: int, y, lab_out, mean, std):
    """Batch ``cursor % n_batches`` of the shard x_u8 [n,H,W,3] -> y [batch,H,W,8] bf16 (+ labels)."""
    assert x_u8.dtype == torch.uint8 and x_u8.shape[-1] == 3 and y.shape[-1] == 8
    img = x_u8.shape[1] * x_u8.shape[2]
    n_batches = x_u8.shape[0] // batch
    assert n_batches >= 1 and y.shape[0] == batch
    N.call("sl_input_norm", p(x_u8), p(labels), p(cursor), n_batches, batch, img, _bf16(y), p(lab_out),
           *[float(v) for v in mean], *[float(v) for v in std], N.stream_ptr())


def input_aug(x_u8, labels, cursor, batch: int, y, lab_out, params_out, mean, std, seed: int = 0,
              shuffle: bool = False, augment: str = "none", pad: int = 4):
    """The training input pipeline (data/augment.py): sample j of the batch at ``cursor`` is a record
    of the shard x_u8 [n,H,W,3] -- drawn through the epoch's permutation with ``shuffle`` -- cropped at
    a random offset out of its zero-padded image and mirrored at random with ``augment="crop-flip"``,
    then normalised as :func:`input_norm` does -> y [batch,H,W,8] bf16 (+ labels).  ``params_out``
    (int32 [batch, 4]) receives each sample's (record, oy, ox, flip)."""
    from ..data import augment as A

    assert x_u8.dtype == torch.uint8 and x_u8.shape[-1] == 3 and y.shape[-1] == 8 and x_u8.is_contiguous()
    n, h, w = x_u8.shape[0], x_u8.shape[1], x_u8.shape[2]
    A.check(augment, pad, min(h, w))
    assert n >= batch and y.shape[0] == batch and tuple(y.shape[1:3]) == (h, w)
    assert labels.dtype == torch.uint8 and labels.numel() >= n and lab_out.numel() >= batch
    assert params_out.dtype == torch.int32 and params_out.numel() == 4 * batch and params_out.is_contiguous()
    assert cursor.dtype == torch.int32
    N.call("sl_input_aug", p(x_u8), p(labels), p(cursor), n, batch, h, w, pad, A.flags(shuffle, augment),
           seed & ((1 << 64) - 1), _bf16(y), p(lab_out), p(params_out), *[float(v) for v in mean],
           *[float(v) for v in std], N.stream_ptr())


def input_mix(x_u8, labels, cursor, batch: int, y, lab_out, params_out, mix_out, table, mean, std, seed: int = 0,
              shuffle: bool = False, augment: str = "none", pad: int = 4, mixup: bool = False, cutmix: bool = False):
    """:func:`input_aug` followed by mixup and / or CutMix (data/augment.py): every sample of the batch
    at ``cursor`` is blended with (``mixup``) or shows a box of (``cutmix``) another sample of the same
    batch, both taken after their own shuffle / crop / flip; with both on the mode is drawn per batch.
    ``table`` (int32 [2, 4096], data/augment.py ``mix_tables``) holds the lambda quantiles of each mode.
    ``params_out`` is :func:`input_aug`'s; ``mix_out`` (int32 [batch, 8]) receives each sample's
    (partner, num, den, mode, x0, y0, x1, y1), num / den the weight of the partner's label."""
    from ..data import augment as A

    assert x_u8.dtype == torch.uint8 and x_u8.shape[-1] == 3 and y.shape[-1] == 8 and x_u8.is_contiguous()
    n, h, w = x_u8.shape[0], x_u8.shape[1], x_u8.shape[2]
    A.check(augment, pad, min(h, w))
    if not (mixup or cutmix):
        raise ValueError("input_mix: neither mixup nor cutmix is on (input_aug is the unmixed pipeline)")
    if batch < 2:
        raise ValueError(f"input_mix: a sample's partner is another sample of its batch (batch >= 2), got {batch}")
    assert n >= batch and y.shape[0] == batch and tuple(y.shape[1:3]) == (h, w)
    assert labels.dtype == torch.uint8 and labels.numel() >= n and lab_out.numel() >= batch
    assert params_out.dtype == torch.int32 and params_out.numel() == 4 * batch and params_out.is_contiguous()
    assert mix_out.dtype == torch.int32 and mix_out.numel() == 8 * batch and mix_out.is_contiguous()
    assert table.dtype == torch.int32 and tuple(table.shape) == (2, A.MIX_L) and table.is_contiguous()
    assert table.device == x_u8.device and cursor.dtype == torch.int32
    modes = (A.MODE_MIXUP if mixup else 0) | (A.MODE_CUTMIX if cutmix else 0)
    N.call("sl_input_mix", p(x_u8), p(labels), p(cursor), n, batch, h, w, pad, A.flags(shuffle, augment),
           seed & ((1 << 64) - 1), p(table), modes, _bf16(y), p(lab_out), p(params_out), p(mix_out),
           *[float(v) for v in mean], *[float(v) for v in std], N.stream_ptr())


def cursor_bump(cursor):
    N.call("sl_cursor_bump", p(cursor), N.stream_ptr())


def bn_finalize(stats, gamma, beta, coef, run_mean, run_var, count, eps=1e-5, momentum=0.1):
    c = gamma.numel()
    N.call("sl_bn_finalize", _f32(stats), _f32(gamma), _f32(beta), _f32(coef), _f32(run_mean), _f32(run_var), c,
           float(count), float(eps), float(momentum), N.stream_ptr())


def bn_apply(x, coef, y, relu=True, res=None, rcoef=None):
    c = x.shape[-1]
    rows = x.numel() // c
    mode = 0 if res is None else (2 if rcoef is not None else 1)
    N.call("sl_bn_apply", _bf16(x), _f32(coef), _bf16(res) if res is not None else None, _f32(rcoef), _bf16(y),
           rows, c, 1 if relu else 0, mode, N.stream_ptr())


def bn_bwd_reduce(dy, y, x, sums, dz_out=None, mask_coef=None, y_mask=None, x2=None, sums2=None):
    """dz = dy * relu'(.) and the per-channel sums for the BN backward.  The ReLU
    mask comes from ``y`` (block outputs with a residual) or, for a plain
    ``y = relu(bn(x))``, from ``x`` and the layer's forward ``mask_coef``
    (scale/shift rows of ``coef``), so ``y`` is never read.  ``y_mask`` is the
    1-bit-per-channel ReLU mask written by :func:`bn_apply_stats` (``mask_out``)
    for block outputs with a residual: 1/16 of the bytes of ``y``.  ``x2``/``sums2``
    add the sums of a second BN fed by the same dz (the downsample shortcut's
    input ``cs``), so dz is not read back for it."""
    c = x.shape[-1]
    rows = x.numel() // c
    assert (y is not None) + (mask_coef is not None) + (y_mask is not None) <= 1
    assert (x2 is None) == (sums2 is None) and (x2 is None or x2.shape == x.shape)
    if y_mask is not None:
        assert y_mask.dtype == torch.uint8 and y_mask.numel() * 8 == x.numel() and y_mask.is_contiguous()
    N.call("sl_bn_bwd_reduce", _bf16(dy), _bf16(y) if y is not None else None, _bf16(x),
           _f32(mask_coef) if mask_coef is not None else None, p(y_mask) if y_mask is not None else None,
           _bf16(dz_out) if dz_out is not None else None, _f32(sums),
           _bf16(x2) if x2 is not None else None, _f32(sums2) if sums2 is not None else None, rows, c,
           N.stream_ptr())


def bn_bwd_finalize(sums, coef, dcoef, grad_gamma, grad_beta, count):
    c = grad_gamma.numel()
    N.call("sl_bn_bwd_finalize", _f32(sums), _f32(coef), _f32(dcoef), _f32(grad_gamma), _f32(grad_beta), c,
           float(count), N.stream_ptr())


def bn_bwd_apply(dy, y, x, dcoef, dx):
    c = x.shape[-1]
    rows = x.numel() // c
    N.call("sl_bn_bwd_apply", _bf16(dy), _bf16(y) if y is not None else None, _bf16(x), _f32(dcoef), _bf16(dx),
           rows, c, N.stream_ptr())


def bn_apply_stats(x, bn, y, count, relu=True, res=None, rbn=None, eps=1e-5, momentum=0.1, mask_out=None,
                   res_relu=False):
    """Fused finalize + apply; ``bn``/``rbn`` expose stats, gamma, beta, coef, run_mean, run_var.
    ``mask_out`` (u8, numel/8) receives bit j of byte q = ``y[8q+j] > 0``.  ``res_relu``: the
    residual is ``relu(rbn(res))`` (a BN-on-load block input, whose BN was published by the
    conv that consumed it; ``rbn``'s coef / running stats are not written here)."""
    if mask_out is not None:
        assert mask_out.dtype == torch.uint8 and mask_out.numel() * 8 == x.numel() and mask_out.is_contiguous()
    c = x.shape[-1]
    rows = x.numel() // c
    mode = 0 if res is None else ((3 if res_relu else 2) if rbn is not None else 1)
    assert not res_relu or rbn is not None
    r = rbn
    N.call("sl_bn_apply_stats", _bf16(x), _f32(bn.stats), _f32(bn.gamma), _f32(bn.beta), _f32(bn.coef),
           _f32(bn.run_mean), _f32(bn.run_var), _bf16(res) if res is not None else None,
           _f32(r.stats) if r else None, _f32(r.gamma) if r else None, _f32(r.beta) if r else None,
           _f32(r.coef) if r else None, _f32(r.run_mean) if r else None, _f32(r.run_var) if r else None,
           _bf16(y), p(mask_out) if mask_out is not None else None, rows, c, 1 if relu else 0, mode, float(count), float(eps), float(momentum), N.stream_ptr())


def bn_bwd_apply_sums(dy, y, x, sums, coef, grad_gamma, grad_beta, dx, mask_coef=None):
    """Fused backward finalize + apply: dx, and dgamma/dbeta accumulated into the flat gradient.
    ``mask_coef`` as in :func:`bn_bwd_reduce`."""
    c = x.shape[-1]
    rows = x.numel() // c
    assert y is None or mask_coef is None
    N.call("sl_bn_bwd_apply_sums", _bf16(dy), _bf16(y) if y is not None else None, _bf16(x),
           _f32(mask_coef) if mask_coef is not None else None, _f32(sums),
           _f32(coef), _f32(grad_gamma), _f32(grad_beta), _bf16(dx), rows, c, float(rows), N.stream_ptr())


def bn_bwd_apply_dual(dz, xa, sums_a, coef_a, gg_a, gb_a, dx_a, xb, sums_b, coef_b, gg_b, gb_b, dx_b):
    """:func:`bn_bwd_apply_sums` for two BNs fed by the same ``dz`` (a downsample
    block's bn2 and shortcut BN), reading ``dz`` once."""
    c = xa.shape[-1]
    rows = xa.numel() // c
    assert xb.shape == xa.shape == dz.shape == dx_a.shape == dx_b.shape
    N.call("sl_bn_bwd_apply_dual", _bf16(dz), _bf16(xa), _f32(sums_a), _f32(coef_a), _f32(gg_a), _f32(gb_a),
           _bf16(dx_a), _bf16(xb), _f32(sums_b), _f32(coef_b), _f32(gg_b), _f32(gb_b), _bf16(dx_b), rows, c,
           float(rows), N.stream_ptr())


def maxpool_fwd(x, y, arg, k=3, s=2, pad=1):
    n, h, w, c = x.shape
    _, oh, ow, _ = y.shape
    N.call("sl_maxpool_fwd", _bf16(x), _bf16(y), p(arg), n, h, w, c, oh, ow, k, s, pad, N.stream_ptr())


def maxpool_bwd(dy, arg, dx, k=3, s=2, pad=1):
    n, h, w, c = dx.shape
    _, oh, ow, _ = dy.shape
    N.call("sl_maxpool_bwd", _bf16(dy), p(arg), _bf16(dx), n, h, w, c, oh, ow, k, s, pad, N.stream_ptr())


def avgpool_fwd(x, y):
    n, h, w, c = x.shape
    N.call("sl_avgpool_fwd", _bf16(x), _bf16(y), n, h * w, c, N.stream_ptr())


def avgpool_bwd(dy, dx):
    n, h, w, c = dx.shape
    N.call("sl_avgpool_bwd", _bf16(dy), _bf16(dx), n, h * w, c, N.stream_ptr())


NARROW_CLASSES = 16  # softmax_ce_kernel: one row on a 16-lane group
WIDE_CLASSES = 256   # softmax_ce_wide_kernel: one row on a wave, four classes per lane


def logit_ld(ncls: int) -> int:
    """Row stride of dlogits for ``ncls`` classes: 16 up to 16 classes, else the next power of two
    ``>= max(32, ncls)`` (the FC data gradient reads dlogits as an image of that many channels)."""
    if isinstance(ncls, bool) or int(ncls) != ncls or not 1 <= ncls <= WIDE_CLASSES:
        raise ValueError(f"classes must be an integer in 1..{WIDE_CLASSES}, got {ncls!r}")
    return 16 if ncls <= NARROW_CLASSES else max(32, 1 << (int(ncls) - 1).bit_length())


def softmax_ce_wide_ws(n: int, ncls: int, device) -> torch.Tensor | None:
    """The bias-gradient workspace of the wide loss for ``n`` rows (None up to 16 classes, where the
    narrow kernel needs none).  It holds nothing between calls."""
    if ncls <= NARROW_CLASSES:
        return None
    words = int(N.lib().sl_softmax_ce_wide_ws_floats(int(n), logit_ld(ncls)))
    return torch.empty(max(words, 1), dtype=torch.float32, device=device)


def _softmax_ce_wide(logits, labels, loss, correct, dlogits, dbias, grad_scale, mix, eps, soft, ws):
    n, ncls = logits.shape
    if ws is None:
        raise ValueError(f"softmax_ce over {ncls} classes needs the bias-gradient workspace (softmax_ce_wide_ws)")
    assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.device == logits.device
    assert labels.dtype == torch.uint8 and labels.numel() >= n
    assert dlogits.numel() >= n * dlogits.shape[-1] and (loss is None or loss.numel() >= n)
    assert correct is None or correct.numel() >= n
    assert dbias is None or dbias.numel() >= ncls
    N.call("sl_softmax_ce_wide", _f32(logits), p(labels), _f32(loss), _f32(correct), _bf16(dlogits),
           dlogits.shape[-1], _f32(dbias), n, ncls, float(grad_scale), p(mix) if mix is not None else None,
           float(eps), 1 if soft else 0, p(ws), int(ws.numel()), N.stream_ptr())


def softmax_ce(logits, labels, loss, correct, dlogits, dbias, grad_scale, ws=None):
    """Softmax cross-entropy of fp32 ``logits`` [n, ncls] against u8 ``labels``: per-row ``loss`` and
    ``correct``, ``dlogits`` (bf16 [n, ldd], zero beyond ncls) scaled by ``grad_scale``, and their row
    sum added into ``dbias``.  Up to 16 classes the narrow kernel; 17..256 the wide one, which needs
    ``ws`` (:func:`softmax_ce_wide_ws`) and ``ldd = logit_ld(ncls)`` or another power of two in
    ``max(32, ncls)..256``."""
    n, ncls = logits.shape
    if ncls > NARROW_CLASSES:
        return _softmax_ce_wide(logits, labels, loss, correct, dlogits, dbias, grad_scale, None, 0.0, False, ws)
    N.call("sl_softmax_ce", _f32(logits), p(labels), _f32(loss), _f32(correct), _bf16(dlogits), dlogits.shape[-1],
           _f32(dbias), n, ncls, float(grad_scale), N.stream_ptr())


def softmax_ce_soft(logits, labels, loss, correct, dlogits, dbias, grad_scale, mix=None, eps: float = 0.0, ws=None):
    """:func:`softmax_ce` against soft targets (data/augment.py ``soft_targets``): row i's target is
    ``(1 - eps)(wa [c = la] + wb [c = lb]) + eps / ncls`` with ``la = labels[i]`` and, from row i of
    ``mix`` (int32 [n, 8], :func:`input_mix`'s ``mix_out``; None = label smoothing alone),
    ``lb = labels[mix[i, 0]]``, ``wb = mix[i, 1] / mix[i, 2]``, ``wa = 1 - wb``.  ``correct`` stays the
    argmax against ``la``: under mixing it is a diagnostic, not an accuracy.  ``ws`` as in
    :func:`softmax_ce`."""
    n, ncls = logits.shape
    if not 0 <= eps < 1:
        raise ValueError(f"label smoothing must be in [0, 1), got {eps!r}")
    assert labels.dtype == torch.uint8 and labels.numel() >= n
    if mix is not None:
        assert mix.dtype == torch.int32 and mix.numel() == 8 * n and mix.is_contiguous()
    if ncls > NARROW_CLASSES:
        return _softmax_ce_wide(logits, labels, loss, correct, dlogits, dbias, grad_scale, mix, eps, True, ws)
    N.call("sl_softmax_ce_soft", _f32(logits), p(labels), _f32(loss), _f32(correct), _bf16(dlogits),
           dlogits.shape[-1], _f32(dbias), n, ncls, float(grad_scale), p(mix) if mix is not None else None,
           float(eps), N.stream_ptr())
