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

* **TrivialAugment Wide** (``auto_augment="trivial-wide"``; after crop / flip, before the mix, whose
  partner is then the partner after its own operation).  ``T = philox4x32_10(t, 0, j, 4; seed)``:
  sample ``j`` gets the one operation ``op = T.x % 14`` of torchvision's ``TrivialAugmentWide`` list at
  strength ``bin = T.y % 31`` (``m = bin / 30``) and sign ``neg = T.z & 1``.  Every constant that
  involves a float is rounded once on the host into :func:`ta_table`; :func:`ta_apply` and
  ``input_ta_kernel`` (csrc/kernels/input_ta.hip) read the same integers and do integer arithmetic
  only, so they agree bit for bit.  The operations are written out at :func:`ta_apply`.

* **RandomResizedCrop + flip** (``augment="rrc-flip"``; in place of crop / flip, ``augment_pad``
  unused).  For try ``k = 0..9``, ``R = philox4x32_10(t, k, j, 5; seed)`` indexes :func:`rrc_table` at
  ``[R.x >> 24][R.y >> 24]``: 256 areas between ``rrc_min_scale`` and 1 of the image by 256 log-uniform
  aspect ratios in 3/4..4/3, each a box ``w | h << 16`` or 0 where the box does not fit.  The first
  entry that fits is the crop, at ``top = R.z % (O - h + 1)``, ``left = R.w % (O - w + 1)``; ten misses
  take the whole image (torchvision's fallback for a square image).  ``flip`` is
  ``philox4x32_10(t, 10, j, 5; seed).x & 1``.  The box is resized back to ``O x O`` bilinearly with
  half-pixel centres, separably, in integers with one rounding (:func:`rrc_apply`); every float of the
  method lives in the table.  ``input_rrc_kernel`` (csrc/kernels/input_rrc.hip) equals it bit for bit.

The shard generator uses Philox's fourth counter word 0 (data/device_synth.py); the streams here
use 1, 2, 3, 4 and 5, so they never collide with it under one seed.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from .device_synth import MASK, philox4x32_10

AUGMENTS = ("none", "crop-flip", "rrc-flip")
STREAM_SHUFFLE, STREAM_CROP, STREAM_MIX = 1, 2, 3
STREAM_TA = 4
STREAM_RRC = 5
RRC_L = 256  # areas, and aspect ratios, of an RRC table (an index is the top 8 bits of a Philox word)
RRC_TRIES = 10
RRC_MIN_HW, RRC_MAX_HW = 4, 256  # input_rrc_kernel: a side that is a multiple of 4 in this range
AUTO_AUGMENTS = ("none", "trivial-wide")
TA_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
          "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")  # torchvision's order
TA_BINS = 31
TA_MAX_PIXELS = 4096  # one workgroup keeps one image in LDS, a packed word per pixel
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
    elif augment != "none":  # ("rrc-flip" has rows of its own: rrc_params)
        raise ValueError(f"batch_params: augment {augment!r} (choose from ('none', 'crop-flip'))")
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


# ---- TrivialAugment Wide ----
def check_ta(auto_augment: str, in_hw: int | None = None) -> None:
    """Refuse what no trainer implements (Config and both trainers call this)."""
    if auto_augment not in AUTO_AUGMENTS:
        raise ValueError(f"unknown auto_augment {auto_augment!r} (choose from {AUTO_AUGMENTS})")
    if auto_augment != "none" and in_hw is not None and in_hw * in_hw > TA_MAX_PIXELS:
        raise ValueError(f"auto_augment: an image of {in_hw} x {in_hw} pixels does not fit the kernel's workgroup "
                         f"(at most {TA_MAX_PIXELS} pixels)")


@functools.lru_cache(maxsize=None)
def ta_table() -> np.ndarray:
    """int32 [14, 31, 2, 8] (op, bin, neg): the constants of every operation at every strength,
    computed in float64 and rounded once.  Ops 1-5 hold (A, B, Cx, D, E, Cy) of the inverse map in
    Q16 (the translations doubled, as the coordinates are); ops 6-9 the blend factor F in column 0;
    Posterize its bit mask; Solarize its threshold; the others nothing."""
    tab = np.zeros((len(TA_OPS), TA_BINS, 2, 8), np.int64)
    q = 65536
    for b in range(TA_BINS):
        m = b / (TA_BINS - 1)
        for neg in (0, 1):
            sg = -1 if neg else 1
            sh = sg * int(np.rint(0.99 * m * q))
            tr = sg * int(np.rint(32.0 * m)) * 2 * q
            th = math.radians(sg * 135.0 * m)
            c, s = int(np.rint(math.cos(th) * q)), int(np.rint(math.sin(th) * q))
            tab[1, b, neg, :6] = (q, sh, 0, 0, q, 0)    # source x = x + s y about the centre
            tab[2, b, neg, :6] = (q, 0, 0, sh, q, 0)    # source y = y + s x
            tab[3, b, neg, :6] = (q, 0, -tr, 0, q, 0)   # the image moves right by k: source x = x - k
            tab[4, b, neg, :6] = (q, 0, 0, 0, q, -tr)
            tab[5, b, neg, :6] = (c, -s, 0, s, c, 0)    # counter-clockwise by theta, as np.rot90 turns
            tab[6:10, b, neg, 0] = 256 + sg * int(np.rint(0.99 * 256.0 * m))
            tab[10, b, neg, 0] = (0xFF << int(np.rint(6.0 * m))) & 0xFF  # keeps 8 - rint(6 m) high bits
            tab[11, b, neg, 0] = 255 - int(np.rint(255.0 * m))
    tab = tab.astype(np.int32)
    tab.setflags(write=False)
    return tab


def ta_params(seed: int, t: int, batch: int) -> np.ndarray:
    """int32 [batch, 4] of (op, bin, neg, 0) at cursor ``t``."""
    r = philox4x32_10(t, 0, np.arange(batch, dtype=np.uint64), STREAM_TA, *_keys(seed))
    out = np.zeros((batch, 4), np.int32)
    out[:, 0] = r[0] % np.uint64(len(TA_OPS))
    out[:, 1] = r[1] % np.uint64(TA_BINS)
    out[:, 2] = r[2] & np.uint64(1)
    return out


def _grey(a: np.ndarray) -> np.ndarray:
    return (77 * a[..., 0] + 150 * a[..., 1] + 29 * a[..., 2] + 128) >> 8


def _ta_one(a: np.ndarray, op: int, e: np.ndarray) -> np.ndarray:
    """One image ``a`` (int64 [H, W, 3], values 0..255) under operation ``op`` with table row ``e``."""
    hh, ww, _ = a.shape
    if op == 0:
        return a
    if op <= 5:  # nearest-neighbour inverse affine map about the centre, black outside
        v, u = np.meshgrid(2 * np.arange(hh) - (hh - 1), 2 * np.arange(ww) - (ww - 1), indexing="ij")
        sx = (e[0] * u + e[1] * v + e[2] + (ww - 1) * 65536 + 65536) >> 17
        sy = (e[3] * u + e[4] * v + e[5] + (hh - 1) * 65536 + 65536) >> 17
        inside = (sx >= 0) & (sx < ww) & (sy >= 0) & (sy < hh)
        out = a[np.clip(sy, 0, hh - 1), np.clip(sx, 0, ww - 1)]
        return np.where(inside[..., None], out, 0)
    if op <= 9:  # blend with a degenerate image d: a at F = 256, d at F = 0, beyond a above 256
        if op == 6:
            d = np.zeros_like(a)
        elif op == 7:
            d = np.broadcast_to(_grey(a)[..., None], a.shape)
        elif op == 8:
            d = np.full_like(a, (int(_grey(a).sum()) + hh * ww // 2) // (hh * ww))
        else:
            d = a.copy()
            if hh > 2 and ww > 2:
                box = sum(a[dy:hh - 2 + dy, dx:ww - 2 + dx] for dy in range(3) for dx in range(3))
                d[1:-1, 1:-1] = (box + 4 * a[1:-1, 1:-1] + 6) // 13
        return np.clip((256 * d + e[0] * (a - d) + 128) >> 8, 0, 255)
    if op == 10:
        return a & e[0]
    if op == 11:
        return np.where(a < e[0], a, 255 - a)
    out = a.copy()
    for c in range(3):
        ch = a[..., c]
        if op == 12:
            lo, hi = int(ch.min()), int(ch.max())
            if hi != lo:
                out[..., c] = ((ch - lo) * 510 + (hi - lo)) // (2 * (hi - lo))
        else:  # PIL's equalize
            h = np.bincount(ch.reshape(-1), minlength=256)
            step = (hh * ww - int(h[np.nonzero(h)[0][-1]])) // 255
            if step:
                lut = np.minimum(255, (step // 2 + np.cumsum(h) - h) // step)
                out[..., c] = lut[ch]
    return out


def ta_apply(a_u8: np.ndarray, ta: np.ndarray, table: np.ndarray | None = None) -> np.ndarray:
    """The u8 [B, H, W, 3] batch after each sample's operation ``ta[j] = (op, bin, neg, 0)``; ``a_u8`` is
    :func:`apply`'s output.  Integers only.  With ``e = table[op, bin, neg]``:

    * 1-5 ShearX, ShearY, TranslateX, TranslateY, Rotate: with the doubled centred coordinates
      ``u = 2x - (W-1)``, ``v = 2y - (H-1)``, output pixel ``(y, x)`` reads source
      ``sx = (A u + B v + Cx + (W-1) 65536 + 65536) >> 17`` and ``sy`` likewise from ``(D, E, Cy)``
      (floor); black outside.  Shear factor ``+-0.99 m``, translation ``+-rint(32 m)`` pixels, rotation
      ``+-135 m`` degrees.
    * 6-9 Brightness, Color, Contrast, Sharpness: ``clamp((256 d + F (a - d) + 128) >> 8, 0, 255)``,
      ``F = 256 +- rint(0.99 * 256 m)``; ``d`` is 0, the grey ``L = (77 r + 150 g + 29 b + 128) >> 8``, the
      image mean of ``L`` (``(sum + HW // 2) // HW``), or the 3x3 smooth ``(sum_9 a + 4 a + 6) // 13`` at
      interior pixels and ``a`` on the border.
    * 10 Posterize keeps ``8 - rint(6 m)`` high bits; 11 Solarize: ``a < th ? a : 255 - a``,
      ``th = 255 - rint(255 m)``.
    * 12 AutoContrast, per channel: ``((a - lo) 510 + (hi - lo)) // (2 (hi - lo))``, unchanged if
      ``hi == lo``.  13 Equalize, per channel, PIL's rule: ``step = (HW - h[largest occupied level]) //
      255``; unchanged if 0, else ``lut[v] = min(255, (step // 2 + sum_{w<v} h[w]) // step)``."""
    a = np.asarray(a_u8)
    if a.ndim != 4 or a.shape[3] != 3 or a.shape[1] * a.shape[2] > TA_MAX_PIXELS or len(ta) != len(a):
        raise ValueError(f"ta_apply: a batch [B, H, W, 3] of at most {TA_MAX_PIXELS} pixels per image and one row of "
                         f"ta per sample, got {a.shape} and {len(ta)} rows")
    tab = (ta_table() if table is None else np.asarray(table)).astype(np.int64)
    out = np.empty(a.shape, np.uint8)
    for j, (op, b, neg, _) in enumerate(np.asarray(ta)):
        out[j] = _ta_one(a[j].astype(np.int64), int(op), tab[op, b, neg])
    return out


# ---- RandomResizedCrop + flip ----
def check_rrc(min_scale: float, in_hw: int | None = None) -> None:
    """Refuse what no trainer implements (Config and both trainers call this)."""
    if not (math.isfinite(min_scale) and 0 < min_scale <= 1):
        raise ValueError(f"rrc_min_scale must be finite and in (0, 1], got {min_scale!r}")
    if in_hw is not None and not (RRC_MIN_HW <= in_hw <= RRC_MAX_HW and in_hw % 4 == 0):
        raise ValueError(f"augment='rrc-flip': the image side must be a multiple of 4 in {RRC_MIN_HW}..{RRC_MAX_HW} "
                         f"(the kernel's four-pixel stores and its LDS band), got {in_hw}")


@functools.lru_cache(maxsize=None)
def rrc_table(O: int, min_scale: float = 0.08) -> np.ndarray:
    """int32 [256, 256] (area, ratio): entry ``(s, r)`` is the box of area ``O O (min_scale +
    (1 - min_scale)(s + 0.5) / 256)`` and aspect ratio ``exp(log(3/4) + (log(4/3) - log(3/4))(r + 0.5) /
    256)`` as ``w | h << 16``, sides rounded to the nearest integer in float64; 0 where a side is 0
    or larger than ``O`` (torchvision redraws)."""
    check_rrc(min_scale)
    u = (np.arange(RRC_L, dtype=np.float64) + 0.5) / RRC_L
    area = (float(O) * O * (min_scale + (1.0 - min_scale) * u))[:, None]
    q = np.exp(math.log(3 / 4) + (math.log(4 / 3) - math.log(3 / 4)) * u)[None, :]
    w, h = np.rint(np.sqrt(area * q)).astype(np.int64), np.rint(np.sqrt(area / q)).astype(np.int64)
    ok = (w > 0) & (w <= O) & (h > 0) & (h <= O)
    tab = np.where(ok, w | (h << 16), 0).astype(np.int32)
    tab.setflags(write=False)
    return tab


def rrc_params(seed: int, t: int, n: int, batch: int, O: int, shuffle: bool, table: np.ndarray) -> np.ndarray:
    """int32 [batch, 8] of (record, top, left, h, w, flip, tries, fallback) at cursor ``t``.  An entry
    of ``table`` whose box does not fit ``O`` counts as 0, as the kernel reads it."""
    out = np.zeros((batch, 8), np.int32)
    out[:, 0] = batch_params(seed, t, n, batch, 0, shuffle, "none")[:, 0]
    out[:, 3:5], out[:, 6:] = O, (RRC_TRIES, 1)  # ten misses: the whole image
    keys, js = _keys(seed), np.arange(batch, dtype=np.uint64)
    tab = np.asarray(table).astype(np.int64).reshape(RRC_L, RRC_L)
    todo = np.ones(batch, bool)
    for k in range(RRC_TRIES):
        r = philox4x32_10(t, k, js, STREAM_RRC, *keys)
        e = tab[(r[0] >> np.uint64(24)).astype(np.int64), (r[1] >> np.uint64(24)).astype(np.int64)]
        w, h = e & 0xFFFF, (e >> 16) & 0xFFFF
        hit = todo & (w > 0) & (w <= O) & (h > 0) & (h <= O)
        top = r[2].astype(np.int64) % np.where(hit, O - h + 1, 1)
        left = r[3].astype(np.int64) % np.where(hit, O - w + 1, 1)
        out[hit] = np.stack([out[:, 0], top, left, h, w, out[:, 5], np.full(batch, k + 1), np.zeros(batch, np.int64)],
                            1)[hit]
        todo &= ~hit
    out[:, 5] = philox4x32_10(t, RRC_TRIES, js, STREAM_RRC, *keys)[0] & np.uint64(1)
    return out


def rrc_taps(n: int, O: int):
    """(i0, i1, f) of the ``O`` output positions along an axis whose crop is ``n`` long: the two source
    taps within the crop and the second one's weight in 0..256.  The centre of output ``i`` lies at
    ``((2i + 1) n - O) / 2O``; with ``num = (2i + 1) n + O`` (never negative), ``s = num // 2O - 1`` is its
    floor and ``f = ((num - (s + 1) 2O) 256 + O) // 2O`` the fraction, rounded to Q8."""
    num = (2 * np.arange(O, dtype=np.int64) + 1) * n + O
    s = num // (2 * O) - 1
    f = ((num - (s + 1) * 2 * O) * 256 + O) // (2 * O)
    return np.clip(s, 0, n - 1), np.clip(s + 1, 0, n - 1), f


def rrc_apply(x_u8: np.ndarray, params: np.ndarray) -> np.ndarray:
    """The u8 [B, O, O, 3] batch of :func:`rrc_params` rows over the shard ``x_u8`` [N, O, O, 3]: each
    box resized to ``O x O``, bilinear with half-pixel centres (``align_corners=False``).  Horizontally
    ``hr = a (256 - fx) + b fx`` (16 bits, exact), then ``(hr0 (256 - fy) + hr1 fy + 32768) >> 16``: one
    rounding.  With ``flip`` output column ``x`` takes the value of column ``O - 1 - x``."""
    x_u8 = np.asarray(x_u8)
    _, hh, O, ch = x_u8.shape
    if hh != O:
        raise ValueError(f"rrc_apply: square images, got {hh} x {O}")
    out = np.empty((len(params), O, O, ch), np.uint8)
    for j, (rec, top, left, h, w, flip, _, _) in enumerate(np.asarray(params)):
        src = x_u8[rec, top:top + h, left:left + w].astype(np.int64)
        x0, x1, fx = rrc_taps(int(w), O)
        y0, y1, fy = rrc_taps(int(h), O)
        hr = src[:, x0] * (256 - fx)[None, :, None] + src[:, x1] * fx[None, :, None]
        v = (hr[y0] * (256 - fy)[:, None, None] + hr[y1] * fy[:, None, None] + 32768) >> 16
        out[j] = v[:, ::-1] if flip else v
    return out
