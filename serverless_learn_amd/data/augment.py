"""Input pipeline of the ResNet trainers: epoch shuffle and random crop + horizontal flip.

This module is the definition.  ``input_aug_kernel`` (csrc/kernels/cnn_aux.hip) and
``CPUResNetTrainer`` match it bit for bit, and everything is a pure function of
``(seed, t, j, N, B, P, flags)`` -- ``t`` the batch cursor the forward pass reads, ``j`` the sample
within the batch -- so a resumed run, a replayed graph and every replica of a group draw the same
batch with no state beyond the cursor that is checkpointed and broadcast already.

With ``N`` records, batch ``B`` and ``nb = N // B``: ``e = t // nb`` is the epoch and ``b = t % nb``
the batch within it.  All arithmetic is on unsigned 32-bit integers.

* **Shuffle.**  Sample ``j`` takes record ``perm_e(b*B + j)``.  ``perm_e`` is a four-round Feistel
  network on ``bits = max(2, bit_length(N - 1))`` rounded up to even, its round keys
  ``philox4x32_10(e, 0, 0, 1; seed)`` and its round function the murmur3 finalizer, cycle-walked
  until the value is below ``N``: a bijection of ``[0, N)``.  An epoch uses the first ``nb*B``
  positions of its order, so every record can be drawn, the ``N % B`` tail too.
* **Crop + flip.**  ``R = philox4x32_10(t, 0, j, 2; seed)``; ``oy = R.x % (2P + 1)``,
  ``ox = R.y % (2P + 1)``, ``flip = R.z & 1``.  Output pixel ``(y, x)`` reads source pixel
  ``(y + oy - P, xs + ox - P)`` with ``xs = W - 1 - x`` if ``flip`` else ``x``: torchvision's
  ``RandomCrop(W, padding=P)`` followed by ``RandomHorizontalFlip``.  Outside the image the source
  is u8 0 in every channel -- black before normalisation.  (``% (2P + 1)`` is biased by about
  2^-29, which is accepted.)

* **Mixup / CutMix** (``mixup_alpha``, ``cutmix_alpha``; after shuffle / crop / flip).  All integer:
  ``M = philox4x32_10(t, 0, 0, 3; seed)`` and ``Nn = philox4x32_10(t, 1, 0, 3; seed)`` are drawn once
  per batch.  ``M.x >> 20`` indexes :func:`mix_table`, the 4096 quantiles of Beta(alpha, alpha) as
  ``k = round(256 lambda)`` and ``c = round(256 sqrt(1 - lambda))``; sample ``j``'s partner is sample
  ``(j + r) % B`` of the same batch, ``r = 1 + M.y % (B - 1)``, taken after its own shuffle / crop /
  flip; with both alphas on the batch is CutMix when ``M.z & 1``.  Mixup: every channel is
  ``(k ua + (256 - k) ub) / 256`` in pixel units (exact in fp32), the partner's label weighs
  ``(256 - k) / 256``.  CutMix: a box of ``((W c + 128) >> 8) x ((H c + 128) >> 8)`` pixels centred at
  ``(Nn.x % W, Nn.y % H)`` and clipped to the image takes the partner's pixels; the partner's label
  weighs the pasted area over ``H W``.  :func:`soft_targets` adds label smoothing:
  ``q = (1 - eps)(wa [c = la] + wb [c = lb]) + eps / ncls``.

The shard generator uses Philox's fourth counter word 0 (data/device_synth.py); the streams here
use 1, 2 and 3, so they never collide with it under one seed.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from .device_synth import MASK, philox4x32_10

AUGMENTS = ("none", "crop-flip")
STREAM_SHUFFLE, STREAM_CROP, STREAM_MIX = 1, 2, 3
MIX_L = 4096  # entries of a mix table (the table index is the top 12 bits of a Philox word)
MODE_MIXUP, MODE_CUTMIX = 1, 2  # column 3 of mix_params; bits of sl_input_mix's modes
FLAG_SHUFFLE, FLAG_CROP_FLIP = 1, 2  # sl_input_aug's flags


def check(augment: str, pad: int, in_hw: int) -> None:
    """Refuse what no trainer implements (both trainers call this at construction)."""
    if augment not in AUGMENTS:
        raise ValueError(f"unknown augment {augment!r} (choose from {AUGMENTS})")
    if not 0 <= pad < in_hw:
        raise ValueError(f"augment_pad must be in [0, {in_hw}), got {pad!r}")


def flags(shuffle: bool, augment: str) -> int:
    return (FLAG_SHUFFLE if shuffle else 0) | (FLAG_CROP_FLIP if augment == "crop-flip" else 0)


def _keys(seed: int) -> tuple[int, int]:
    return seed & MASK, (seed >> 32) & MASK


def fmix32(x: np.ndarray) -> np.ndarray:
    """murmur3's 32-bit finalizer on uint64 arrays holding 32-bit values."""
    m = np.uint64(MASK)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & m
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & m
    return x ^ (x >> np.uint64(16))


def half_bits(n: int) -> int:
    """Width of one Feistel half for ``n`` records."""
    bits = max(2, int(n - 1).bit_length())
    return (bits + 1) // 2


def perm(seed: int, epoch: int, n: int, q) -> np.ndarray:
    """``perm_epoch(q)`` for every position in ``q`` (each in ``[0, n)``): int64, same shape."""
    q = np.asarray(q)
    if q.size and (q.min() < 0 or q.max() >= n):
        raise ValueError("perm: positions must lie in [0, n)")
    h = np.uint64(half_bits(n))
    mask = np.uint64((1 << int(h)) - 1)
    keys = [np.uint64(int(k)) for k in philox4x32_10(epoch, 0, 0, STREAM_SHUFFLE, *_keys(seed))]
    v = q.astype(np.uint64).reshape(-1).copy()
    todo = np.ones(v.shape, bool)
    while todo.any():
        w = v[todo]
        left, right = w >> h, w & mask
        for k in keys:
            left, right = right, left ^ (fmix32((right + k) & np.uint64(MASK)) & mask)
        v[todo] = (left << h) | right
        todo &= v >= np.uint64(n)
    return v.astype(np.int64).reshape(q.shape)


def draws(seed: int, t: int, batch: int, pad: int):
    """(oy, ox, flip) of the ``batch`` samples at cursor ``t``: three int64 arrays."""
    r = philox4x32_10(t, 0, np.arange(batch, dtype=np.uint64), STREAM_CROP, *_keys(seed))
    span = np.uint64(2 * pad + 1)
    return (r[0] % span).astype(np.int64), (r[1] % span).astype(np.int64), (r[2] & np.uint64(1)).astype(np.int64)


def batch_params(seed: int, t: int, n: int, batch: int, pad: int, shuffle: bool, augment: str) -> np.ndarray:
    """int32 [batch, 4] of (record, oy, ox, flip) at cursor ``t``; a part that is off leaves its
    columns at (b*B + j, pad, pad, 0)."""
    nb = n // batch
    if nb < 1:
        raise ValueError("shard smaller than one batch")
    e, b = divmod(int(t), nb)
    out = np.empty((batch, 4), np.int32)
    pos = b * batch + np.arange(batch)
    out[:, 0] = perm(seed, e, n, pos) if shuffle else pos
    out[:, 1:] = (pad, pad, 0)
    if augment == "crop-flip":
        out[:, 1], out[:, 2], out[:, 3] = draws(seed, t, batch, pad)
    elif augment != "none":
        raise ValueError(f"unknown augment {augment!r} (choose from {AUGMENTS})")
    return out


def apply(x_u8: np.ndarray, params: np.ndarray, pad: int) -> np.ndarray:
    """The u8 [B, H, W, 3] batch the network should see: records ``params[:, 0]`` of the shard
    ``x_u8`` [N, H, W, 3], shifted, flipped and zero-padded.  Exact: the gather is in u8 space."""
    x_u8 = np.asarray(x_u8)
    _, hh, ww, _ = x_u8.shape
    padded = np.zeros((len(params), hh + 2 * pad, ww + 2 * pad, x_u8.shape[3]), x_u8.dtype)
    padded[:, pad:pad + hh, pad:pad + ww] = x_u8[params[:, 0]]
    out = np.empty((len(params), hh, ww, x_u8.shape[3]), x_u8.dtype)
    for j, (_, oy, ox, flip) in enumerate(params):
        # output (y, x) <- source (y + oy - pad, xs + ox - pad): the crop of the mirrored columns
        win = padded[j, oy:oy + hh, ox:ox + ww]
        out[j] = win[:, ::-1] if flip else win
    return out


# ---- label smoothing, mixup and CutMix ----
def check_mix(label_smoothing: float, mixup_alpha: float, cutmix_alpha: float, batch: int | None = None) -> None:
    """Refuse what no trainer implements (Config and both trainers call this)."""
    if not 0 <= label_smoothing < 1:  # NaN included
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing!r}")
    for name, a in (("mixup_alpha", mixup_alpha), ("cutmix_alpha", cutmix_alpha)):
        if not (math.isfinite(a) and a >= 0):
            raise ValueError(f"{name} must be finite and >= 0 (0 = off), got {a!r}")
    if batch is not None and batch < 2 and (mixup_alpha > 0 or cutmix_alpha > 0):
        raise ValueError("mixup_alpha / cutmix_alpha: a sample's partner is another sample of its batch "
                         f"(batch >= 2), got batch {batch}")


def _betacf(a: float, x: np.ndarray) -> np.ndarray:
    """Continued fraction of the incomplete beta function I_x(a, a) (modified Lentz), x <= 1/2."""
    tiny = 1e-300
    qab, qap, qam = 2.0 * a, a + 1.0, a - 1.0
    c = np.ones_like(x)
    d = 1.0 - qab * x / qap
    d = 1.0 / np.where(np.abs(d) < tiny, tiny, d)
    h = d.copy()
    for m in range(1, 500):
        m2 = 2 * m
        for aa in (m * (a - m) * x / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + aa * d
            d = 1.0 / np.where(np.abs(d) < tiny, tiny, d)
            c = 1.0 + aa / c
            c = np.where(np.abs(c) < tiny, tiny, c)
            h = h * d * c
        if np.all(np.abs(d * c - 1.0) < 4e-16):
            break
    return h


def _betainc_sym(a: float, x: np.ndarray) -> np.ndarray:
    """Regularised incomplete beta function I_x(a, a) for 0 <= x <= 1/2, float64."""
    x = np.asarray(x, np.float64)
    safe = np.where(x > 0, x, 0.25)
    front = np.exp(math.lgamma(2 * a) - 2 * math.lgamma(a) + a * (np.log(safe) + np.log1p(-safe)))
    return np.where(x > 0, front * _betacf(a, safe) / a, 0.0)


@functools.lru_cache(maxsize=None)
def _lower_quantiles(alpha: float, n: int) -> np.ndarray:
    """Quantiles of Beta(alpha, alpha) at (i + 0.5) / n for i < n / 2: all below 1/2, by bisection."""
    if not (math.isfinite(alpha) and alpha > 0) or n < 2 or n % 2:
        raise ValueError(f"beta_quantiles: alpha must be finite and > 0 and the length even, got {alpha!r}, {n!r}")
    p = (np.arange(n // 2) + 0.5) / n
    lo, hi = np.zeros(n // 2), np.full(n // 2, 0.5)
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        below = _betainc_sym(alpha, mid) < p
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    q = 0.5 * (lo + hi)
    q.setflags(write=False)
    return q


def beta_quantiles(alpha: float, n: int = MIX_L) -> np.ndarray:
    """The ``n`` quantiles of Beta(alpha, alpha) at ``(i + 0.5) / n``, float64: the lower half by
    bisection of the regularised incomplete beta function, the upper half its mirror image."""
    q = _lower_quantiles(float(alpha), int(n))
    return np.concatenate([q, 1.0 - q[::-1]])


def mix_table(alpha: float, n: int = MIX_L) -> np.ndarray:
    """int32 [n]: entry i packs ``k = floor(256 Q_i + 0.5)`` (lambda = k / 256) in its low 16 bits
    and ``c = floor(256 sqrt(1 - Q_i) + 0.5)`` (CutMix's side ratio c / 256) in its high 16 bits."""
    q = _lower_quantiles(float(alpha), int(n))
    k = np.floor(256.0 * q + 0.5).astype(np.int64)
    k = np.concatenate([k, 256 - k[::-1]])  # the mirror image exactly: k_i + k_(n-1-i) = 256
    c = np.floor(256.0 * np.sqrt(np.concatenate([1.0 - q, q[::-1]])) + 0.5).astype(np.int64)
    return (k | (c << 16)).astype(np.int32)


def mix_tables(mixup_alpha: float, cutmix_alpha: float) -> np.ndarray:
    """int32 [2, MIX_L], what sl_input_mix indexes: row 0 is mixup's table, row 1 CutMix's (a mode
    that is off leaves its row at k = 256, c = 0: no mixing)."""
    off = np.full(MIX_L, 256, np.int32)
    return np.stack([mix_table(mixup_alpha) if mixup_alpha > 0 else off,
                     mix_table(cutmix_alpha) if cutmix_alpha > 0 else off])


def mix_params(seed: int, t: int, batch: int, H: int, W: int, mixup_alpha: float, cutmix_alpha: float,
               tables: np.ndarray | None = None) -> np.ndarray:
    """int32 [batch, 8] of (pj, num, den, mode, x0, y0, x1, y1) at cursor ``t``: sample j's partner,
    the partner's label weight num / den, mode 1 = mixup (box columns 0) or 2 = CutMix with the
    pasted box [x0, x1) x [y0, y1).  ``tables`` replaces :func:`mix_tables` (tests)."""
    check_mix(0.0, mixup_alpha, cutmix_alpha, batch)
    if not (mixup_alpha > 0 or cutmix_alpha > 0):
        raise ValueError("mix_params: neither mixup_alpha nor cutmix_alpha is on")
    if tables is None:
        tables = mix_tables(mixup_alpha, cutmix_alpha)
    m = [int(v) for v in philox4x32_10(t, 0, 0, STREAM_MIX, *_keys(seed))]
    nn = [int(v) for v in philox4x32_10(t, 1, 0, STREAM_MIX, *_keys(seed))]
    r = 1 + m[1] % (batch - 1)
    if mixup_alpha > 0 and cutmix_alpha > 0:
        mode = MODE_CUTMIX if m[2] & 1 else MODE_MIXUP
    else:
        mode = MODE_CUTMIX if cutmix_alpha > 0 else MODE_MIXUP
    entry = int(tables[mode - 1][m[0] >> 20])
    k, c = entry & 0xFFFF, (entry >> 16) & 0xFFFF
    out = np.zeros((batch, 8), np.int32)
    out[:, 0] = (np.arange(batch) + r) % batch
    out[:, 3] = mode
    if mode == MODE_MIXUP:
        out[:, 1], out[:, 2] = 256 - k, 256
    else:
        cx, cy = nn[0] % W, nn[1] % H
        bw, bh = (W * c + 128) >> 8, (H * c + 128) >> 8
        x0, x1 = max(cx - bw // 2, 0), min(cx - bw // 2 + bw, W)
        y0, y1 = max(cy - bh // 2, 0), min(cy - bh // 2 + bh, H)
        if bw == 0 or bh == 0:
            x0 = y0 = x1 = y1 = 0
        out[:, 1], out[:, 2] = (x1 - x0) * (y1 - y0), H * W
        out[:, 4:] = (x0, y0, x1, y1)
    return out


def mix_apply(xa_u8: np.ndarray, mix: np.ndarray) -> np.ndarray:
    """float32 [B, H, W, 3] in pixel units from the already augmented u8 batch ``xa_u8`` (exact:
    mixup's ``k ua + (256 - k) ub`` is below 2^16 and the division by 256 a shift)."""
    xa = np.asarray(xa_u8).astype(np.int64)
    xb = xa[mix[:, 0]]
    if int(mix[0, 3]) == MODE_MIXUP:
        k = (256 - mix[:, 1].astype(np.int64)).reshape(-1, 1, 1, 1)
        return ((k * xa + (256 - k) * xb) / 256.0).astype(np.float32)
    out = xa.copy()
    for j, (_, _, _, _, x0, y0, x1, y1) in enumerate(mix):
        out[j, y0:y1, x0:x1] = xb[j, y0:y1, x0:x1]
    return out.astype(np.float32)


def soft_targets(labels: np.ndarray, mix: np.ndarray | None, eps: float, ncls: int) -> np.ndarray:
    """float64 [B, ncls] targets ``q = (1 - eps)(wa [c = la] + wb [c = lb]) + eps / ncls`` of the
    batch's own ``labels``; ``mix`` None is smoothing alone."""
    la = np.asarray(labels).astype(np.int64)
    q = np.zeros((len(la), ncls), np.float64)
    rows = np.arange(len(la))
    if mix is None:
        q[rows, la] = 1.0
    else:
        wb = mix[:, 1].astype(np.float64) / mix[:, 2].astype(np.float64)
        np.add.at(q, (rows, la), 1.0 - wb)
        np.add.at(q, (rows, la[mix[:, 0]]), wb)
    return (1.0 - eps) * q + eps / ncls
