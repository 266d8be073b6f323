"""Top-k sparse gossip on the CPU: wire form, selection order, exchange rules, worker plumbing."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from serverless_learn_amd.config import Config
from serverless_learn_amd.parallel.gossip import GossipState, exact_exchange, select_topk
from serverless_learn_amd.proto import messages as pb
from serverless_learn_amd.runtime.local_cluster import fast_config
from serverless_learn_amd.runtime.transport import Channels, RpcServer
from serverless_learn_amd.runtime.worker import Worker
from serverless_learn_amd.wire import codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- codec
GOLDEN = bytes.fromhex("1208" "01000000" "05000000" "1a08" "0000803f" "000000c0" "20ac02")


def test_sparse_update_golden_bytes():
    # index [1, 5] | value [1.0, -2.0] | sparse_len 300 (varint ac 02); delta absent
    msg = codec.encode_sparse_update(np.array([1, 5], np.uint32), np.array([1.0, -2.0], np.float32), 300)
    assert msg == GOLDEN
    assert pb.Update(sparse_index=np.array([1, 5], "<u4").tobytes(), sparse_value=np.array([1, -2], "<f4").tobytes(),
                     sparse_len=300).SerializeToString() == GOLDEN


def test_sparse_update_round_trip():
    rng = np.random.default_rng(0)
    for n, count in ((1, 1), (7, 0), (1000, 37), (70_000, 70_000)):
        idx = np.sort(rng.choice(n, size=count, replace=False)).astype(np.uint32)
        val = rng.standard_normal(count).astype(np.float32)
        kind, i2, v2, n2 = codec.decode_update_any(codec.encode_sparse_update(idx, val, n))
        assert kind == "sparse" and n2 == n and i2.dtype == np.uint32 and v2.dtype == np.float32
        np.testing.assert_array_equal(i2, idx)
        np.testing.assert_array_equal(v2.view(np.uint32), val.view(np.uint32))
    kind, dense = codec.decode_update_any(codec.encode_update(np.array([1.5, -2.0])))
    assert kind == "dense" and dense.dtype == np.float64
    np.testing.assert_array_equal(dense, [1.5, -2.0])
    kind, dense = codec.decode_update_any(b"")
    assert kind == "dense" and dense.size == 0


def _raw(index_bytes: bytes, value_bytes: bytes, n: int) -> bytes:
    return pb.Update(sparse_index=index_bytes, sparse_value=value_bytes, sparse_len=n).SerializeToString()


def _u4(*xs):
    return np.array(xs, "<u4").tobytes()


def test_sparse_update_rejections():
    two = np.array([1.0, 2.0], "<f4").tobytes()
    assert codec.decode_update_any(_raw(_u4(1, 2), two, 3))[0] == "sparse"
    bad = {
        "index bytes % 4": _raw(_u4(1, 2)[:7], two, 3),
        "value bytes % 4": _raw(_u4(1, 2), two[:6], 3),
        "unequal counts": _raw(_u4(1, 2, 3), two, 9),
        "repeated index": _raw(_u4(2, 2), two, 9),
        "descending index": _raw(_u4(2, 1), two, 9),
        "index == sparse_len": _raw(_u4(1, 3), two, 3),
        "truncated": GOLDEN[:-6],
    }
    for why, msg in bad.items():
        with pytest.raises(ValueError):
            codec.decode_update_any(msg)
            pytest.fail(why)
    # sparse iff sparse_len is present and non-zero: without it the (empty) delta is what counts
    assert codec.decode_update_any(_raw(_u4(2, 1), two, 0))[0] == "dense"


def test_dense_decoders_and_original_parsers_read_a_sparse_message_as_empty():
    assert codec.decode_update(GOLDEN, "float64").size == 0
    u = pb.Update.FromString(GOLDEN)
    assert len(u.delta) == 0 and u.sparse_len == 300
    assert np.frombuffer(u.sparse_index, "<u4").tolist() == [1, 5]
    assert np.frombuffer(u.sparse_value, "<f4").tolist() == [1.0, -2.0]
    # an "old" Update parser (only delta = 1), in the style of test_wire.py
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

    fdp = descriptor_pb2.FileDescriptorProto(name="old_update.proto", package="old", syntax="proto3")
    m = fdp.message_type.add(name="Update")
    m.field.add(name="delta", number=1, type=1, label=3)
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    Old = message_factory.GetMessageClass(pool.FindMessageTypeByName("old.Update"))
    assert list(Old.FromString(GOLDEN).delta) == []
    got = {f.name: f.number for f in pb.PROTO.messages["Update"]}
    assert got == {"delta": 1, "sparse_index": 2, "sparse_value": 3, "sparse_len": 4}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_sparse_codec_program_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_wire_sparse")
    core = os.path.join(ROOT, "csrc", "core")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I" + core, os.path.join(core, "test_wire_sparse.cpp"),
                    os.path.join(core, "wire.cpp"), "-o", exe], check=True, timeout=300)
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0 and proc.stdout.split() == ["ok"], proc.stderr[-3000:]


# ---------------------------------------------------------------- selection order
def _brute(d: np.ndarray, k: int) -> np.ndarray:
    key = d.astype(np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    order = np.lexsort((np.arange(d.size), -key.astype(np.int64)))  # key descending, then index ascending
    order = order[key[order] != 0][:k]
    return np.sort(order).astype(np.uint32)


def _cases():
    rng = np.random.default_rng(3)
    n = 257
    zeros = np.zeros(n, np.float32)
    few = zeros.copy()
    few[[3, 100, 256]] = [1.0, -2.0, 0.5]
    pairs = np.repeat(rng.standard_normal(n // 2 + 1).astype(np.float32), 2)[:n] * np.where(np.arange(n) % 2, -1, 1)
    odd = rng.standard_normal(n).astype(np.float32)
    odd[[0, 9]] = np.inf, -np.inf
    odd[5] = np.nan
    odd[10:20] = np.arange(1, 11, dtype=np.uint32).view(np.float32)      # denormals
    odd[20:24] = [0.0, -0.0, 0.0, -0.0]
    return {"random": rng.standard_normal(n).astype(np.float32), "all_equal": np.full(n, -0.75, np.float32),
            "pairs": pairs.astype(np.float32), "mostly_zero": few, "zeros": zeros, "nonfinite_denormal": odd}


@pytest.mark.parametrize("name", list(_cases()))
def test_select_topk_matches_a_brute_force_lexsort(name):
    d = _cases()[name]
    n = d.size
    for k in (1, 7, math.ceil(0.01 * n), 100, n):
        got = select_topk(d, k)
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(got, _brute(d, k), err_msg=f"{name} k={k}")
    if name == "all_equal":
        np.testing.assert_array_equal(select_topk(d, 9), np.arange(9))       # the lowest indices win
    if name == "mostly_zero":
        np.testing.assert_array_equal(select_topk(d, 7), [3, 100, 256])      # fewer than k
    if name == "zeros":
        assert select_topk(d, n).size == 0
    if name == "nonfinite_denormal":
        np.testing.assert_array_equal(select_topk(d, 3), [0, 5, 9])          # nan, then the infinities
        full = select_topk(d, n)
        assert set(range(10, 20)) <= set(full.tolist()) and not set(range(20, 24)) & set(full.tolist())
    if name == "pairs":
        top = int(np.argmax(np.abs(d)))
        assert select_topk(d, 1).tolist() == [top - top % 2]                # +x before -x: the lower index


def test_make_sparse_delta_sends_values_and_advances_old():
    m = np.array([1.0, 5.0, -3.0, 2.0, 2.0], np.float32)
    g = GossipState(torch.from_numpy(m.copy()), 0.5)
    g.old.zero_()
    i, v = g.make_sparse_delta(3)
    assert i.dtype == np.uint32 and v.dtype == np.float32
    assert i.tolist() == [1, 2, 3] and v.tolist() == [5.0, -3.0, 2.0]
    assert g.old.tolist() == [0.0, 5.0, -3.0, 2.0, 0.0] and g.model.tolist() == m.tolist()
    i, v = g.make_sparse_delta(3)            # the rest goes out later
    assert i.tolist() == [0, 4] and v.tolist() == [1.0, 2.0]
    assert g.make_sparse_delta(3)[0].size == 0
    with pytest.raises(ValueError):
        GossipState(torch.zeros(4), compat=True).make_sparse_delta(2)
    with pytest.raises(ValueError):
        GossipState(torch.zeros(0, dtype=torch.float64), growable=True).serve_sparse([], [], 2)
    with pytest.raises(ValueError):
        g.serve_sparse([0], [1.0], 2, sparse_len=6)
    with pytest.raises(ValueError):
        g.absorb_sparse([5], [1.0])


# ---------------------------------------------------------------- exchange rules
def _dyadic(rng, n):
    return (rng.integers(-4095, 4096, n) / 1024.0).astype(np.float32)   # multiples of 2^-10, |x| < 4


def _state(m, o, a=0.5):
    g = GossipState(torch.from_numpy(m.copy()), a)
    g.old.copy_(torch.from_numpy(o))
    return g


@pytest.mark.parametrize("n,k", [(1000, 1000), (1000, 64), (257, 1)])
def test_sparse_exchanges_equal_one_dense_echo_free_exchange(n, k):
    rng = np.random.default_rng(n + k)
    mA, oA, mB, oB = (_dyadic(rng, n) for _ in range(4))
    A, B = _state(mA, oA), _state(mB, oB)
    for _ in range(math.ceil(n / k)):
        for x, y in ((A, B), (B, A)):
            i, v = x.make_sparse_delta(k)
            x.absorb_sparse(*y.serve_sparse(i, v, k, sparse_len=n))
    wantA, _, wantB, _, _ = exact_exchange(mA.astype(np.float64), oA.astype(np.float64), mB.astype(np.float64),
                                           oB.astype(np.float64), 0.5, compat=False)
    np.testing.assert_array_equal(A.model.numpy(), wantA.astype(np.float32))
    np.testing.assert_array_equal(B.model.numpy(), wantB.astype(np.float32))
    assert torch.equal(A.old, A.model) and torch.equal(B.old, B.model)      # both residuals exactly zero
    # the dense exchange itself, through the dense code path
    A2, B2 = _state(mA, oA), _state(mB, oB)
    d = A2.make_delta()
    A2.absorb(B2.serve(d), d)
    np.testing.assert_array_equal(A.model.numpy(), A2.model.numpy())
    np.testing.assert_array_equal(B.model.numpy(), B2.model.numpy())


def test_unsend_restores_old_bit_for_bit():
    rng = np.random.default_rng(8)
    m, o = _dyadic(rng, 500), _dyadic(rng, 500)
    g = _state(m, o)
    i, v = g.make_sparse_delta(40)
    assert i.size == 40 and not np.array_equal(g.old.numpy(), o)
    g.unsend(i, v)
    np.testing.assert_array_equal(g.old.numpy().view(np.uint32), o.view(np.uint32))
    np.testing.assert_array_equal(g.model.numpy().view(np.uint32), m.view(np.uint32))


def test_a_serve_during_the_rpc_neither_loses_nor_double_counts():
    """A sends to B; while that RPC is in flight C's exchange is served by A; then B's reply lands."""
    rng = np.random.default_rng(9)
    n, k, a = 300, 300, 0.5
    mA, oA, mB, oB, mC, oC = (_dyadic(rng, n) for _ in range(6))
    A, B, C = _state(mA, oA), _state(mB, oB), _state(mC, oC)
    dA, dB, dC = (x.astype(np.float64) - y for x, y in ((mA, oA), (mB, oB), (mC, oC)))
    iA, vA = A.make_sparse_delta(k)                    # on the wire to B
    iC, vC = C.make_sparse_delta(k)
    rAC = A.serve_sparse(iC, vC, k, sparse_len=n)      # lands in between
    assert rAC[0].size == 0                            # A's progress is already on the wire: not shared twice
    C.absorb_sparse(*rAC)
    A.absorb_sparse(*B.serve_sparse(iA, vA, k, sparse_len=n))
    np.testing.assert_array_equal(A.model.numpy(), (mA + a * dC + a * dB).astype(np.float32))
    np.testing.assert_array_equal(B.model.numpy(), (mB + a * dA).astype(np.float32))
    np.testing.assert_array_equal(C.model.numpy(), mC)  # nothing of A's reached C, and nothing was invented
    for g in (A, B, C):
        assert torch.equal(g.old, g.model)


# ---------------------------------------------------------------- configuration
def test_config_gossip_topk_and_its_refusals(monkeypatch):
    assert Config().gossip_topk == 0.0 and Config().gossip_k(1000) == 0
    c = Config(sync="gossip", gossip_topk=0.05)
    assert c.gossip_k(269_322) == 13_467 and c.gossip_k(10) == 1 and Config(gossip_topk=1.0).gossip_k(10) == 10
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gossip_topk"):
            Config(sync="gossip", gossip_topk=bad)
    for kw in (dict(sync="ps"), dict(model="simulate"), dict(sync="gossip", gossip_compat=True)):
        with pytest.raises(ValueError, match="gossip_topk"):
            Config(gossip_topk=0.1, **kw)
        with pytest.raises(ValueError, match="gossip_topk"):
            Config.from_env(gossip_topk=0.1, **kw)
    monkeypatch.setenv("SL_GOSSIP_TOPK", "0.25")
    assert Config.from_env(sync="gossip").gossip_topk == 0.25
    import argparse

    from serverless_learn_amd.config import add_cli_args, from_args

    ap = argparse.ArgumentParser()
    add_cli_args(ap)
    assert from_args(ap.parse_args(["--gossip-topk", "0.5", "--sync", "gossip"])).gossip_topk == 0.5
    with pytest.raises(ValueError, match="gossip_topk"):
        from_args(ap.parse_args(["--gossip-topk", "0.5", "--sync", "ps"]))
    cfg = fast_config(sync="gossip")
    cfg.gossip_topk = 0.1
    cfg.gossip_compat = True                       # set after construction: the worker checks again
    with pytest.raises(ValueError, match="gossip_topk"):
        Worker("127.0.0.1:0", cfg)


# ---------------------------------------------------------------- worker plumbing
def _worker(**kw) -> Worker:
    # no master: the view is set by hand and gossip_once is called by hand (the loop never fires)
    cfg = fast_config(sync="gossip", master_addr="127.0.0.1:1", gossip_interval_ms=10 ** 8, **kw)
    w = Worker("127.0.0.1:0", cfg).start()
    with w.train_lock:
        w._ensure_trainer()
    return w


def _record(w: Worker) -> list:
    seen = []
    inner = w.channels.unary

    def unary(target, service, method, request, **kw):
        raw = inner(target, service, method, request, **kw)
        seen.append((method, len(request), len(raw)))
        return raw

    w.channels.unary = unary
    return seen


def test_two_sparse_workers_exchange_few_bytes():
    a, b = _worker(gossip_topk=0.05), _worker(gossip_topk=0.05)
    try:
        n = a.gossip.model.numel()
        k = a.cfg.gossip_k(n)
        assert k == math.ceil(0.05 * n) and b.gossip.model.numel() == n
        rng = np.random.default_rng(0)
        stepA = torch.from_numpy(_dyadic(rng, n))
        stepB = torch.from_numpy(_dyadic(rng, n))
        a0, b0 = a.gossip.model.clone(), b.gossip.model.clone()
        a.gossip.model += stepA
        b.gossip.model += stepB
        dA = (a.gossip.model.double() - a.gossip.old.double()).float().numpy()
        dB = (b.gossip.model.double() - b.gossip.old.double()).float().numpy()
        a.view["peers"] = [a.addr, b.addr]
        seen = _record(a)
        assert a.gossip_once()
        (method, sent, received), = seen
        assert method == "ExchangeUpdates"
        assert 8 * k < sent <= 8 * k + 16 and 8 * k < received <= 8 * k + 16   # dense: 8 * n each way
        iA, iB = select_topk(dA, k), select_topk(dB, k)
        wantA = (a0 + stepA).double().numpy()
        wantA[iB] += 0.5 * dB[iB]
        wantB = (b0 + stepB).double().numpy()
        wantB[iA] += 0.5 * dA[iA]
        np.testing.assert_array_equal(a.gossip.model.numpy(), wantA.astype(np.float32))
        np.testing.assert_array_equal(b.gossip.model.numpy(), wantB.astype(np.float32))
        assert a.gossip.exchanges == 1 and b.gossip.exchanges == 1
        # a failed RPC takes the advance of `old` back
        old = a.gossip.old.clone()
        a.view["peers"] = [a.addr, "127.0.0.1:1"]
        assert a.gossip_once() is False
        # (these parameters are not dyadic: the rounding of o + v - v stays behind as ordinary residual)
        assert torch.allclose(a.gossip.old, old, rtol=0, atol=1e-6)
        assert not torch.equal(a.gossip.old, a.gossip.model) and a.gossip.exchanges == 1
    finally:
        a.stop(leave=False)
        b.stop(leave=False)


def test_sparse_client_absorbs_the_dense_reply_of_a_dense_only_peer():
    a = _worker(gossip_topk=0.05)
    n = a.gossip.model.numel()
    dense_reply = _dyadic(np.random.default_rng(1), n).astype(np.float64)
    got = []

    def dense_only(request, context):
        got.append(codec.decode_update(request, "float64"))  # all a dense-only build reads: an empty delta
        return codec.encode_update(dense_reply)

    srv = RpcServer("127.0.0.1:0", max_workers=2)
    srv.add_service("Worker", {"ExchangeUpdates": dense_only})
    srv.start()
    try:
        a.gossip.model += torch.from_numpy(_dyadic(np.random.default_rng(2), n))
        before = a.gossip.model.clone()
        a.view["peers"] = [a.addr, srv.addr]
        assert a.gossip_once()
        assert got[0].size == 0
        want = (before.double().numpy() + 0.5 * dense_reply).astype(np.float32)
        np.testing.assert_array_equal(a.gossip.model.numpy(), want)
    finally:
        srv.stop()
        a.stop(leave=False)


def test_sparse_client_mixes_in_nothing_from_a_reply_for_another_length():
    a = _worker(gossip_topk=0.05)
    n = a.gossip.model.numel()
    srv = RpcServer("127.0.0.1:0", max_workers=2)
    srv.add_service("Worker", {"ExchangeUpdates": lambda r, c: codec.encode_sparse_update([0], [1.0], n + 1)})
    srv.start()
    try:
        a.gossip.model += torch.from_numpy(_dyadic(np.random.default_rng(6), n))
        before = a.gossip.model.clone()
        twin = GossipState(before.clone(), a.cfg.learn_rate)
        twin.old.copy_(a.gossip.old)
        a.view["peers"] = [a.addr, srv.addr]
        assert a.gossip_once() is False
        assert torch.equal(a.gossip.model, before) and a.gossip.exchanges == 0
        # the peer did take what was sent, so it stays shared: old is not taken back
        assert twin.make_sparse_delta(a.cfg.gossip_k(n))[0].size == a.cfg.gossip_k(n)
        assert torch.equal(a.gossip.old, twin.old) and not torch.equal(a.gossip.old, before)
    finally:
        srv.stop()
        a.stop(leave=False)


def test_dense_client_of_a_sparse_enabled_worker_gets_the_dense_bytes():
    b = _worker(gossip_topk=0.05)
    ch = Channels()
    try:
        n = b.gossip.model.numel()
        b.gossip.model += torch.from_numpy(_dyadic(np.random.default_rng(3), n))
        twin = GossipState(b.gossip.model.clone(), b.cfg.learn_rate)
        twin.old.copy_(b.gossip.old)
        delta = _dyadic(np.random.default_rng(4), n).astype(np.float64)
        raw = ch.unary(b.addr, "Worker", "ExchangeUpdates", codec.encode_update(delta))
        assert raw == codec.encode_update(twin.serve(delta)) and len(raw) > 8 * n
        assert torch.equal(b.gossip.model, twin.model) and torch.equal(b.gossip.old, twin.old)
        # and a sparse request to a worker without a k of its own is answered with as many entries as it brought
        c = _worker()
        try:
            c.gossip.model += torch.from_numpy(_dyadic(np.random.default_rng(5), n))
            idx = np.arange(0, 40, 2, dtype=np.uint32)
            raw = ch.unary(c.addr, "Worker", "ExchangeUpdates",
                           codec.encode_sparse_update(idx, np.ones(20, np.float32), n))
            kind, ri, rv, rn = codec.decode_update_any(raw)
            assert kind == "sparse" and rn == n and ri.size == 20
        finally:
            c.stop(leave=False)
    finally:
        ch.close()
        b.stop(leave=False)
