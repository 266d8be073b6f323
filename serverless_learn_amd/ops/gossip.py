"""K7: fused gossip delta-apply on a device-resident model (csrc/kernels/elementwise.hip) and the
top-k sparse select / scatter (csrc/kernels/gossip_sparse.hip)."""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N


def delta_apply(model: torch.Tensor, old: torch.Tensor, din: torch.Tensor | None, alpha: float,
                dout: torch.Tensor | None) -> None:
    """m += alpha*din (f64, may be shorter than m); dout = m - o (f64); o = m."""
    assert model.is_cuda and model.dtype == torch.float32 and old.dtype == torch.float32
    assert model.is_contiguous() and old.is_contiguous() and old.numel() == model.numel()
    n = model.numel()
    kin = 0
    if din is not None:
        din = din.to(torch.float64).contiguous()
        kin = din.numel()
        if kin > n:
            raise ValueError("incoming delta longer than the model")
    if dout is not None:
        assert dout.dtype == torch.float64 and dout.numel() >= n and dout.is_contiguous()
    N.call("sl_gossip_apply", N.ptr(model), N.ptr(old), N.ptr(din), kin, float(alpha), N.ptr(dout), n,
           N.stream_ptr())


def absorb(model: torch.Tensor, old: torch.Tensor, r: torch.Tensor, alpha: float,
           sent: torch.Tensor | None) -> None:
    """m += alpha*r; o += sent + alpha*r (sent omitted: o += alpha*r). r, sent: f64, may be short."""
    assert model.is_cuda and model.dtype == torch.float32 and old.dtype == torch.float32
    assert model.is_contiguous() and old.is_contiguous() and old.numel() == model.numel()
    n = model.numel()
    r = r.to(torch.float64).contiguous()
    if sent is not None:
        sent = sent.to(torch.float64).contiguous()
    kr, ks = r.numel(), (0 if sent is None else sent.numel())
    if kr > n or ks > n:
        raise ValueError("reply or sent delta longer than the model")
    N.call("sl_gossip_absorb", N.ptr(model), N.ptr(old), N.ptr(r), kr, float(alpha), N.ptr(sent), ks, n,
           N.stream_ptr())


def _check_state(model: torch.Tensor, old: torch.Tensor) -> int:
    assert model.is_cuda and model.dtype == torch.float32 and old.dtype == torch.float32
    assert model.is_contiguous() and old.is_contiguous() and old.numel() == model.numel()
    return model.numel()


def topk_workspace(n: int, device) -> torch.Tensor:
    """The select's scratch for an n-element model (the f32 delta, histograms, per-workgroup
    counts).  Allocate once per model, not per call."""
    nbytes = N.lib().sl_gossip_topk_workspace(int(n))
    return torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=device)


def topk_out(k: int, device) -> torch.Tensor:
    """Device outputs of one select of up to k entries: word 0 the count, then k indices, then k values."""
    return torch.empty(4 + 2 * int(k), dtype=torch.int32, device=device)


def topk_select(model: torch.Tensor, old: torch.Tensor, k: int, workspace: torch.Tensor, out: torch.Tensor):
    """The at most k largest |m - o| (exact; ties to the lower index; zeros never), ascending by
    index, and ``o[index] += value``.  Returns host arrays ``(uint32 index, float32 value)``:
    only the count and the selected entries cross to the host."""
    n = _check_state(model, old)
    k = min(int(k), n)
    if k <= 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.float32)
    assert workspace.is_cuda and workspace.numel() * 4 >= N.lib().sl_gossip_topk_workspace(n)
    assert out.is_cuda and out.dtype == torch.int32 and out.numel() >= 4 + 2 * k
    index, value = out[4:4 + k], out[4 + k:4 + 2 * k]
    N.call("sl_gossip_topk", N.ptr(model), N.ptr(old), n, k, N.ptr(index), N.ptr(value), N.ptr(out),
           N.ptr(workspace), N.stream_ptr())
    count = int(out[0].item())
    if not 0 <= count <= k:
        raise RuntimeError(f"sl_gossip_topk returned count {count} for k {k}")
    host = torch.cat((index[:count], value[:count])).cpu().numpy()
    return host[:count].view(np.uint32).copy(), host[count:].view(np.float32).copy()


def scatter(model: torch.Tensor, old: torch.Tensor, index, value, alpha: float, sign_o_only: int = 0) -> None:
    """``sign_o_only == 0``: m[index] += alpha*value and o[index] += alpha*value (absorb_sparse).
    Otherwise o[index] += sign*value only (unsend: -1).  Indices are unique and < n."""
    n = _check_state(model, old)
    idx = np.ascontiguousarray(index, dtype=np.uint32)
    val = np.ascontiguousarray(value, dtype=np.float32)
    if idx.size != val.size:
        raise ValueError("sparse index and value differ in count")
    if idx.size == 0:
        return
    if idx.size > n or int(idx.max()) >= n:
        raise ValueError("sparse index past the model")
    dev = torch.from_numpy(np.concatenate((idx.view(np.int32), val.view(np.int32)))).to(model.device)
    N.call("sl_gossip_scatter", N.ptr(model), N.ptr(old), N.ptr(dev[:idx.size]), N.ptr(dev[idx.size:]),
           idx.size, n, float(alpha), int(sign_o_only), N.stream_ptr())
