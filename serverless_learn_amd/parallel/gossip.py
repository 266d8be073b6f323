"""Asynchronous gossip model averaging.

Reference behaviour (broken as written, intent reconstructed in SURVEY.md §3.4):

* client (/root/reference/src/worker.cc:194-219 + :145-172): every
  GOSSIP_INTERVAL pick a random peer, send ``d = m - o``, receive ``r``,
  ``m += alpha * r``, then ``o = m``;
* server (/root/reference/src/worker.cc:81-100): grow ``m``/``o`` with zeros
  to ``len(d)``, ``m += alpha * d``, reply ``r = m - o``, ``o = m``.

With dA = mA - oA and dB = mB - oB that gives
``mB' = mB + a*dA``, ``r = dB + a*dA``, ``mA' = mA + a*dB + a^2*dA`` -- the
initiator re-absorbs a^2 of its own delta (the "echo").  ``compat=True``
reproduces that bit-exactly; the default echo-free client applies
``a*(r - a*d) = a*dB``.

The state lives wherever the model lives: a torch tensor on the GPU (the
delta-apply is then one fused HIP kernel, ``ops.gossip.delta_apply``: f64
wire values in, f64 reply out, f32 model) or a float64/float32 CPU tensor.
Callers serialize access with the training step (the reference mutated the
vectors from three threads unlocked).

Top-k sparse exchange (new, echo-free mode only): a message carries the at most
``k`` entries of ``m - o`` of largest magnitude as (index, f32 value) pairs, and
``o`` -- which tracks exactly what has been shared -- is the error feedback: it
advances by what goes on the wire when it goes (``make_sparse_delta``; ``unsend``
if the RPC fails) and by what is received (``absorb_sparse``), so whatever is not
sent stays in ``m - o`` for a later message.  The server replies with its own top-k
taken before mixing the request in (``serve_sparse``), so there is no echo to
remove.  On the GPU the selection is ``ops.gossip.topk_select`` (an exact radix
select, csrc/kernels/gossip_sparse.hip); the CPU path below is the same rule in
numpy and is what the kernels are tested against.
"""
from __future__ import annotations

import threading

import numpy as np
import torch


class GossipState:
    def __init__(self, model: torch.Tensor, alpha: float = 0.5, compat: bool = False,
                 growable: bool = False):
        """``model`` is the live flat parameter tensor (mutated in place).

        ``growable`` models (the reference-style simulated vector, CPU only)
        are re-allocated with zeros to the length of a longer incoming update,
        as worker.cc:85-89 does; a trainer-owned model has a fixed size.
        """
        self.model = model
        self.growable = growable
        self.old = model.detach().clone()
        self.alpha = float(alpha)
        self.compat = compat
        self.lock = threading.RLock()
        self.exchanges = 0
        self.serves = 0  # server-side exchanges (each sets o = m)
        self._serves_at_send = 0
        self._topk_ws = None   # device scratch of the sparse select, allocated once (ops.gossip.topk_workspace)
        self._topk_ws_n = 0
        self._topk_out = None

    # -- helpers -------------------------------------------------------------
    def _grow(self, n: int) -> None:
        """Reference semantics: both vectors grow with zeros to the incoming length."""
        if n <= self.model.numel():
            return
        if not self.growable:
            raise ValueError(f"incoming update has {n} elements, model has {self.model.numel()}")
        k = self.model.numel()
        m = torch.zeros(n, dtype=self.model.dtype, device=self.model.device)
        o = torch.zeros_like(m)
        m[:k] = self.model
        o[:k] = self.old
        self.model, self.old = m, o

    def _use_kernel(self) -> bool:
        return self.model.is_cuda

    # -- client side -----------------------------------------------------------
    def make_delta(self) -> np.ndarray:
        """d = m - o (float64, as it goes on the wire).

        Remembers how many server-side exchanges had happened, so ``absorb`` can
        tell whether ``o`` moved while the RPC was in flight."""
        with self.lock:
            self._serves_at_send = self.serves
            return (self.model.double() - self.old.double()).cpu().numpy()

    def absorb(self, reply: np.ndarray, sent: np.ndarray) -> None:
        """Apply the peer's reply (worker.cc:155-164) and advance ``o``.

        The reference then sets ``o = m`` (:215).  Training keeps stepping while the
        RPC is in flight, so ``m`` already holds progress that was never sent; copying
        it into ``o`` would drop it from every later exchange.  ``o`` instead advances
        by exactly what was shared: ``o += sent + a*r``.  If this worker served an
        exchange in the meantime, that serve already set ``o = m`` (its reply carried
        everything, ``sent`` included), so only ``a*r`` is added.  With no concurrent
        steps both rules give ``o = m``, so the exchange math of SURVEY.md §3.4 is
        unchanged.

        ``compat`` keeps the reference's ``o = m`` (worker.cc:215) exactly, so progress made
        while the RPC was in flight is dropped from later exchanges there too -- compat mode
        reproduces the reference, including that loss."""
        with self.lock:
            r = torch.from_numpy(np.asarray(reply, dtype=np.float64))
            self._grow(r.numel())
            a = self.alpha
            s = torch.from_numpy(np.asarray(sent, dtype=np.float64))
            if not self.compat and s.numel() == r.numel():
                r = r - a * s  # remove the echo of our own delta: a*(r - a*d) = a*dB
            if self.serves != self._serves_at_send or s.numel() > self.model.numel():
                s = None  # o was reset by a serve in between: `sent` is already accounted for
            if self._use_kernel():
                from ..ops import gossip as gk

                gk.absorb(self.model, self.old, r.to(self.model.device), a,
                          None if s is None else s.to(self.model.device))
            else:
                n = r.numel()
                m = self.model[:n]
                m.copy_((m.double() + a * r).to(m.dtype))
                o = self.old.double()
                if s is not None:
                    o[:s.numel()] += s
                o[:n] += a * r
                self.old.copy_(o.to(self.old.dtype))
            if self.compat:
                self.old.copy_(self.model)  # worker.cc:215, o = m
            self.exchanges += 1

    # -- server side -----------------------------------------------------------
    def serve(self, delta: np.ndarray) -> np.ndarray:
        """m += a*d; reply r = m - o; o = m (worker.cc:81-100)."""
        with self.lock:
            d = torch.from_numpy(np.asarray(delta, dtype=np.float64))
            self._grow(d.numel())
            a = self.alpha
            if self._use_kernel():
                from ..ops import gossip as gk

                out = torch.empty(self.model.numel(), dtype=torch.float64, device=self.model.device)
                gk.delta_apply(self.model, self.old, d.to(self.model.device), a, out)
                reply = out.cpu().numpy()
            else:
                n = d.numel()
                m = self.model
                m[:n].copy_((m[:n].double() + a * d).to(m.dtype))
                reply = (m.double() - self.old.double()).numpy()
                self.old.copy_(m)
            self.serves += 1
            self.exchanges += 1
            return reply


    # -- top-k sparse exchange (echo-free only) -----------------------------------
    # ``old`` is the error feedback: whatever is not sent stays in m - o and goes out later.
    def _sparse_check(self) -> None:
        if self.compat:
            raise ValueError("sparse gossip is echo-free only: compat reproduces the reference byte for byte")
        if self.growable:
            raise ValueError("a growable model is never sparse")

    def _check_index(self, index, value):
        idx = np.ascontiguousarray(index, dtype=np.uint32).ravel()
        val = np.ascontiguousarray(value, dtype=np.float32).ravel()
        if idx.size != val.size:
            raise ValueError("sparse index and value differ in count")
        if idx.size and int(idx.max()) >= self.model.numel():
            raise ValueError(f"sparse index {int(idx.max())} past the model's {self.model.numel()} elements")
        return idx, val

    def _add_at(self, t: torch.Tensor, idx: np.ndarray, inc: np.ndarray) -> None:
        """t[idx] = dtype(double(t[idx]) + inc) on a CPU tensor (inc: float64)."""
        i = torch.from_numpy(idx.astype(np.int64))
        t[i] = (t[i].double() + torch.from_numpy(inc)).to(t.dtype)

    def make_sparse_delta(self, k: int):
        """The at most ``k`` entries of ``d = float32(double(m) - double(o))`` of largest magnitude:
        ``(uint32 index ascending, float32 value)``, and ``o[index] += value`` in the same call.

        The order is by the bit pattern of ``|d|`` as uint32, larger first (so non-finite values
        first), equal magnitudes to the lower index; ``d == 0`` is never sent, so fewer than
        ``k`` may come back.  ``o`` advances when the values go on the wire, not when the reply
        arrives: a serve landing while the RPC is in flight can neither share the same progress
        twice nor over-advance ``o``.  If the RPC fails, :meth:`unsend` takes it back."""
        self._sparse_check()
        with self.lock:
            n = self.model.numel()
            k = max(0, min(int(k), n))
            if self._use_kernel():
                from ..ops import gossip as gk

                if self._topk_ws is None or self._topk_ws_n != n:
                    self._topk_ws, self._topk_ws_n = gk.topk_workspace(n, self.model.device), n
                if self._topk_out is None or self._topk_out.numel() < 4 + 2 * k:
                    self._topk_out = gk.topk_out(k, self.model.device)
                return gk.topk_select(self.model, self.old, k, self._topk_ws, self._topk_out)
            d = (self.model.double() - self.old.double()).float().numpy()
            idx = select_topk(d, k)
            val = d[idx]
            self._add_at(self.old, idx, val.astype(np.float64))
            return idx, val

    def unsend(self, index, value) -> None:
        """Take back a :meth:`make_sparse_delta` whose RPC failed: ``o[index] -= value``.  Any
        rounding left over is ordinary residual and goes out later."""
        with self.lock:
            idx, val = self._check_index(index, value)
            if self._use_kernel():
                from ..ops import gossip as gk

                gk.scatter(self.model, self.old, idx, val, 1.0, sign_o_only=-1)
            else:
                self._add_at(self.old, idx, -val.astype(np.float64))

    def absorb_sparse(self, index, value) -> None:
        """``m[index] += a*value`` and the same to ``o``: what was received is common knowledge."""
        self._sparse_check()
        with self.lock:
            idx, val = self._check_index(index, value)
            if self._use_kernel():
                from ..ops import gossip as gk

                gk.scatter(self.model, self.old, idx, val, self.alpha)
            else:
                inc = self.alpha * val.astype(np.float64)
                self._add_at(self.model, idx, inc)
                self._add_at(self.old, idx, inc)
            self.exchanges += 1

    def serve_sparse(self, index_in, value_in, k: int, sparse_len: int | None = None):
        """Server side: the reply is this side's own progress, taken BEFORE the incoming delta is
        mixed in, so it carries no echo and the client removes none; then the delta is absorbed."""
        self._sparse_check()
        with self.lock:
            if sparse_len is not None and int(sparse_len) != self.model.numel():
                raise ValueError(f"sparse update addresses {int(sparse_len)} elements, model has {self.model.numel()}")
            idx, val = self._check_index(index_in, value_in)
            reply = self.make_sparse_delta(k)
            self.absorb_sparse(idx, val)
            return reply


def select_topk(d: np.ndarray, k: int) -> np.ndarray:
    """Indices (uint32, ascending) of the at most ``k`` non-zero entries of the float32 vector
    ``d`` with the largest magnitude bits; equal magnitudes go to the lower index."""
    key = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    nz = np.flatnonzero(key)
    if k < nz.size:
        order = np.argsort(-key[nz].astype(np.int64), kind="stable")[:k]
        nz = np.sort(nz[order])
    return nz[:max(0, k)].astype(np.uint32)


def exact_exchange(mA, oA, mB, oB, alpha=0.5, compat=True):
    """Closed form of one exchange A->B, for tests."""
    dA, dB = mA - oA, mB - oB
    mB2 = mB + alpha * dA
    r = dB + alpha * dA
    mA2 = mA + alpha * r if compat else mA + alpha * dB
    return mA2, mA2.copy(), mB2, mB2.copy(), r
