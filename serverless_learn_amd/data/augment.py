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

The shard generator uses Philox's fourth counter word 0 (data/device_synth.py); the two streams
here use 1 and 2, so they never collide with it under one seed.
"""
from __future__ import annotations

import numpy as np

from .device_synth import MASK, philox4x32_10

AUGMENTS = ("none", "crop-flip")
STREAM_SHUFFLE, STREAM_CROP = 1, 2
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
