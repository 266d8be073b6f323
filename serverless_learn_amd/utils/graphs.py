"""Captured-graph lifetime for the fused trainers: a replaced graph is retired, not destroyed.

Destroying a hipGraphExec waits for its launches to finish, and the destructor runs when the
last Python reference goes -- with the GIL held.  A trainer used to drop its graph on any state
change (``self.graph = None`` in ``load_shard``, ``enable_xgmi``, the runtime's checkpoint
load).  When a replay was still spinning on a dead xGMI peer (the update kernel's 10 s
timeout), that assignment blocked the whole process for up to 10 s: the gRPC threads could not
answer the master's CheckUp, and the master evicted two healthy survivors (the
``test_gpu_workers_kill_one_respawn_with_xgmi`` failure in ``profiles/r06_elastic``).

So ``graph`` / ``graph_unrolled`` are slots whose setter keeps the replaced graph in a retired
list.  :meth:`GraphSlots.reap_graphs` frees that list after ``torch.cuda.synchronize``, which
waits with the GIL released.  Trainers call it where they sync anyway: ``capture()`` and
``drop_graphs()``.  Nothing is destroyed while a launch may still be in flight.
"""
from __future__ import annotations

import torch


def _slot(name: str) -> property:
    key = "_slot_" + name

    def get(self):
        return self.__dict__.get(key)

    def put(self, g) -> None:
        old = self.__dict__.get(key)
        if old is not None and old is not g:
            self.__dict__.setdefault("_retired_graphs", []).append(old)
        self.__dict__[key] = g

    return property(get, put)


class GraphSlots:
    """Mixin: ``graph`` and ``graph_unrolled`` retire what they replace (see module doc)."""

    graph = _slot("graph")
    graph_unrolled = _slot("graph_unrolled")

    @property
    def retired_graphs(self) -> int:
        return len(self.__dict__.get("_retired_graphs", ()))

    def reap_graphs(self, sync: bool = True) -> None:
        """Free the retired graphs.  ``sync`` first waits for the device (GIL released), so
        their destructors find nothing in flight; pass False only when the caller has just
        synchronized."""
        retired = self.__dict__.get("_retired_graphs")
        if not retired:
            return
        if sync and self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        retired.clear()


class GraphedStep(GraphSlots):
    """A fused trainer's ``step`` over its ``_step_eager``: eager, or the replay of a captured graph."""

    def step(self) -> None:
        if self.graph is not None:
            self.graph.replay()
            return
        self._step_eager()

    def _capture_steps(self, k: int = 1):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(k):
                self._step_eager()
        return g

    def capture(self, warmup: int = 2) -> None:
        """Capture one step into a hipGraph (kernels only, or kernels + RCCL), after ``warmup`` eager
        steps on a side stream.  Graphs replaced since the last capture are freed first, after a
        device sync (module doc)."""
        self.reap_graphs()
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._step_eager()
        torch.cuda.current_stream(self.device).wait_stream(s)
        self.graph = self._capture_steps()

    def drop_graphs(self) -> None:
        """Release every captured step graph after the device has finished with them.  A
        graph may hold a communicator's kernels: the runtime calls this before it re-forms or
        tears down the group, so no replay is in flight when the old
        communicator goes away and the k-step graph is not left alive holding it."""
        if self.graph is not None or self.retired_graphs:  # steps() ignores graph_unrolled once graph is None
            torch.cuda.synchronize(self.device)
        self.graph = None
        self.graph_unrolled = None
        self.reap_graphs(sync=False)
