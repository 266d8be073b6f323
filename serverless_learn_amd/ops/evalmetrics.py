"""Held-out evaluation metrics: the definition, and the launcher of the kernel that computes them.

:func:`eval_reference` is the specification (float64 and integers, on the CPU); the CPU trainers
run it and ``eval_accum_kernel`` (csrc/kernels/eval_metrics.hip, :func:`eval_accum`) is tested
against it field by field, exactly.

For row ``i`` with logits ``z`` over ``ncls`` classes (up to 16 in ``eval_accum_kernel`` and the names
without a suffix; up to 256 in ``eval_accum_wide_kernel`` and the ``*_wide`` names, whose device block is
``int64 [8 + ncls * ncls]``), label ``l`` (a label ``>= ncls`` counts
as 0, as in ``softmax_ce_kernel``) and ``loss_i`` the fp32 per-row loss the forward pass wrote:

* the row is **bad** when a logit or the loss is not finite or ``|loss_i| >= 2^16``; a bad row adds
  to ``n`` and ``bad`` only;
* ``pred`` is the lowest index among the maxima of ``z``;
  ``rank = #{c : z_c > z_l or (z_c == z_l and c < l)}`` is the number of classes ahead of the label;
* ``top1 += (rank == 0)`` (the same as ``pred == l``), ``topk += (rank < k)``,
  ``confusion[l][pred] += 1``, ``loss_fix += rint(float64(loss_i) * 2^24)`` (to nearest even).

Everything accumulated is an integer, so sums do not depend on order, reports over disjoint record
sets add field by field, and the GPU result is the same from call to call and in both kernel builds.
Nothing overflows an int64 while ``n <= 2^22`` (``|loss_fix| < 2^22 * 2^40``); larger sets are refused.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

MAX_CLASSES = 16
MAX_RECORDS = 1 << 22
LOSS_FIX = float(1 << 24)       # loss_fix is the loss in units of 2^-24
LOSS_BAD = float(1 << 16)       # |loss| at or past this marks a bad row
ACC_HEAD = 8                    # counters in front of the confusion matrix in the device block
ACC_LEN = ACC_HEAD + MAX_CLASSES * MAX_CLASSES
WIDE_CLASSES = 256              # eval_accum_wide_kernel: the u8 label's range; its block is [8 + ncls * ncls]


def check_topk(topk, ncls: int) -> int:
    if isinstance(topk, bool) or int(topk) != topk or not 1 <= topk <= ncls:
        raise ValueError(f"topk must be an integer in 1..{ncls}, got {topk!r}")
    return int(topk)


def check_records(n: int) -> int:
    if n < 1:
        raise ValueError("evaluation set is empty")
    if n > MAX_RECORDS:
        raise ValueError(f"evaluation set of {n} records: at most {MAX_RECORDS} (the int64 loss sum)")
    return int(n)


@dataclass
class EvalReport:
    n: int
    bad: int
    top1: int
    topk: int
    k: int
    loss_fix: int
    confusion: np.ndarray  # int64 [ncls, ncls], [label][prediction]

    @property
    def good(self) -> int:
        return self.n - self.bad

    @property
    def loss(self) -> float:
        return self.loss_fix / LOSS_FIX / self.good if self.good else float("nan")

    @property
    def accuracy(self) -> float:
        return self.top1 / self.good if self.good else float("nan")

    @property
    def topk_accuracy(self) -> float:
        return self.topk / self.good if self.good else float("nan")

    @property
    def per_class_recall(self) -> list:
        """confusion[c][c] over the good rows labelled c (NaN for a class with none)."""
        rows = self.confusion.sum(axis=1)
        return [int(self.confusion[c, c]) / int(rows[c]) if rows[c] else float("nan")
                for c in range(self.confusion.shape[0])]

    def __add__(self, other: "EvalReport") -> "EvalReport":
        if self.k != other.k or self.confusion.shape != other.confusion.shape:
            raise ValueError("reports of different k or class count do not add")
        return EvalReport(self.n + other.n, self.bad + other.bad, self.top1 + other.top1, self.topk + other.topk,
                          self.k, self.loss_fix + other.loss_fix, self.confusion + other.confusion)

    def __eq__(self, other) -> bool:
        return (isinstance(other, EvalReport)
                and (self.n, self.bad, self.top1, self.topk, self.k, self.loss_fix)
                == (other.n, other.bad, other.top1, other.topk, other.k, other.loss_fix)
                and np.array_equal(self.confusion, other.confusion))

    def as_dict(self) -> dict:
        return {"n": self.n, "bad": self.bad, "top1": self.top1, "topk": self.topk, "k": self.k,
                "loss_fix": self.loss_fix, "loss": self.loss, "accuracy": self.accuracy,
                "topk_accuracy": self.topk_accuracy, "per_class_recall": self.per_class_recall,
                "confusion": self.confusion.tolist()}

    def all_bad(self) -> "EvalReport":
        """The same records with every row counted as bad (the MLP's W1 overflow rule)."""
        return EvalReport(self.n, self.n, 0, 0, self.k, 0, np.zeros_like(self.confusion))


def _np(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a).astype(dtype, copy=False)


def eval_reference(logits, labels, loss_rows, ncls: int, topk: int, wide: bool = False) -> EvalReport:
    """The report of rows ``logits[i, :ncls]`` / ``labels[i]`` / ``loss_rows[i]`` (module docstring).
    ``wide``: up to :data:`WIDE_CLASSES` classes (``eval_accum_wide_kernel``'s range)."""
    top = WIDE_CLASSES if wide else MAX_CLASSES
    if not 1 <= ncls <= top:
        raise ValueError(f"ncls must be in 1..{top}, got {ncls}")
    topk = check_topk(topk, ncls)
    z = _np(logits, np.float64)
    z = z.reshape(-1, z.shape[-1])[:, :ncls] if z.size else z.reshape(0, ncls)
    lab = _np(labels, np.int64).reshape(-1)
    lo32 = _np(loss_rows, np.float32).reshape(-1)
    n = z.shape[0]
    if lab.shape[0] != n or lo32.shape[0] != n:
        raise ValueError("logits, labels and loss_rows disagree on the number of rows")
    if n > MAX_RECORDS:
        raise ValueError(f"{n} rows: at most {MAX_RECORDS}")
    lo = lo32.astype(np.float64)
    lab = np.where(lab < ncls, lab, 0)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(z).all(axis=1) | ~np.isfinite(lo) | (np.abs(lo) >= LOSS_BAD)
    good = ~bad
    zg, lg, sg = z[good], lab[good], lo[good]  # the good rows' logits, labels and losses
    cls = np.arange(ncls, dtype=np.int64)[None, :]
    pred = zg.argmax(axis=1).astype(np.int64) if zg.size else np.zeros(0, np.int64)  # the first maximum
    zl = np.take_along_axis(zg, lg[:, None], axis=1) if zg.size else zg.reshape(-1, 1)
    rank = ((zg > zl) | ((zg == zl) & (cls < lg[:, None]))).sum(axis=1)
    conf = np.zeros((ncls, ncls), np.int64)
    np.add.at(conf, (lg, pred), 1)
    loss_fix = sum(int(v) for v in np.rint(sg * LOSS_FIX))  # python integers: no int64 wrap on the way
    return EvalReport(int(n), int(bad.sum()), int((rank == 0).sum()), int((rank < topk).sum()), topk, loss_fix, conf)


def report_from_acc(acc, ncls: int, topk: int) -> EvalReport:
    """The report held by a device block (``int64 [8 + 256]``, :func:`eval_accum`): one copy to the host."""
    a = _np(acc, np.int64).reshape(-1)
    conf = a[ACC_HEAD:ACC_LEN].reshape(MAX_CLASSES, MAX_CLASSES)[:ncls, :ncls].copy()
    return EvalReport(int(a[0]), int(a[1]), int(a[2]), int(a[3]), int(topk), int(a[4]), conf)


# ---- the kernel ------------------------------------------------------------------------------
def new_acc(device) -> torch.Tensor:
    return torch.zeros(ACC_LEN, dtype=torch.int64, device=device)


def eval_accum(logits: torch.Tensor, labels: torch.Tensor, loss_rows: torch.Tensor, n_valid: int, ncls: int,
               topk: int, acc: torch.Tensor) -> None:
    """Add the metrics of rows ``[0, n_valid)`` into ``acc`` (one launch of ``eval_accum_kernel`` on the
    current stream; the caller zeroes ``acc`` once per evaluation).  ``logits`` fp32 ``[rows, ld]``,
    ``labels`` u8 ``[rows]``, ``loss_rows`` fp32 ``[rows]``."""
    from . import _native as N

    rows = int(logits.shape[0])
    if (logits.dtype != torch.float32 or loss_rows.dtype != torch.float32 or labels.dtype != torch.uint8
            or acc.dtype != torch.int64):
        raise TypeError("eval_accum: fp32 logits and loss rows, u8 labels, an int64 block")
    if logits.dim() != 2 or logits.stride(1) != 1 or not labels.is_contiguous() or not loss_rows.is_contiguous():
        raise ValueError("eval_accum: row-major logits, contiguous labels and loss rows")
    if labels.numel() < rows or loss_rows.numel() < rows or acc.numel() < ACC_LEN or not acc.is_contiguous():
        raise ValueError("eval_accum: a buffer is shorter than the rows")
    N.call("sl_eval_accum", N.ptr(logits), int(logits.stride(0)), N.ptr(labels), N.ptr(loss_rows), rows, int(n_valid),
           int(ncls), int(topk), N.ptr(acc), N.stream_ptr())


# ---- up to 256 classes: a block of 8 + ncls * ncls words, the confusion matrix at stride ncls ----
def _check_wide(ncls) -> int:
    if isinstance(ncls, bool) or int(ncls) != ncls or not 1 <= ncls <= WIDE_CLASSES:
        raise ValueError(f"ncls must be an integer in 1..{WIDE_CLASSES}, got {ncls!r}")
    return int(ncls)


def acc_len_wide(ncls: int) -> int:
    ncls = _check_wide(ncls)
    return ACC_HEAD + ncls * ncls


def new_acc_wide(device, ncls: int) -> torch.Tensor:
    return torch.zeros(acc_len_wide(ncls), dtype=torch.int64, device=device)


def report_from_acc_wide(acc, ncls: int, topk: int) -> EvalReport:
    """The report held by a wide device block (``int64 [8 + ncls * ncls]``, :func:`eval_accum_wide`)."""
    n = acc_len_wide(ncls)
    a = _np(acc, np.int64).reshape(-1)
    if a.shape[0] < n:
        raise ValueError(f"a block of {a.shape[0]} words for {ncls} classes: {n} needed")
    conf = a[ACC_HEAD:n].reshape(ncls, ncls).copy()
    return EvalReport(int(a[0]), int(a[1]), int(a[2]), int(a[3]), int(topk), int(a[4]), conf)


def eval_accum_wide(logits: torch.Tensor, labels: torch.Tensor, loss_rows: torch.Tensor, n_valid: int, ncls: int,
                    topk: int, acc: torch.Tensor) -> None:
    """:func:`eval_accum` over up to 256 classes: one launch of ``eval_accum_wide_kernel`` adds the rows
    ``[0, n_valid)`` into ``acc`` (:func:`new_acc_wide`)."""
    from . import _native as N

    rows = int(logits.shape[0])
    if (logits.dtype != torch.float32 or loss_rows.dtype != torch.float32 or labels.dtype != torch.uint8
            or acc.dtype != torch.int64):
        raise TypeError("eval_accum_wide: fp32 logits and loss rows, u8 labels, an int64 block")
    if logits.dim() != 2 or logits.stride(1) != 1 or not labels.is_contiguous() or not loss_rows.is_contiguous():
        raise ValueError("eval_accum_wide: row-major logits, contiguous labels and loss rows")
    if (labels.numel() < rows or loss_rows.numel() < rows or acc.numel() < acc_len_wide(ncls)
            or not acc.is_contiguous()):
        raise ValueError("eval_accum_wide: a buffer is shorter than the rows, or the block than 8 + ncls^2 words")
    N.call("sl_eval_accum_wide", N.ptr(logits), int(logits.stride(0)), N.ptr(labels), N.ptr(loss_rows), rows,
           int(n_valid), int(ncls), int(topk), N.ptr(acc), N.stream_ptr())
