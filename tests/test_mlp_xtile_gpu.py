"""The tiled form of the resident u8 shard (xt[rows / 64][13][64][64], 4 KB bricks) and its two
consumers: the re-layout is exact, and the rows kernel and the weight gradient compute from the
bricks, bit for bit, what they compute from the row-major shard.

The shapes are the smallest that can go wrong: 64 rows (one row block, the 64-row tile), 128
(two bricks per workgroup), a cursor past batch 0 (base arithmetic), columns >= 768 (last
chunk and pad), 192 rows (an odd row-block count beside the 128-row tile)."""
import functools

import numpy as np
import pytest
import torch

from serverless_learn_amd.models import mlp as M

gpu = pytest.mark.gpu

D_IN, NCHUNK, BRICK = M.D_IN, M.D_IN_PAD // 64, 64 * 64


def tile_index(rows):
    """Flat byte offset into the row-major [rows][784] shard of every byte of the tiled form
    xt[rows / 64][13][64][64]; -1 at the pad columns 784..831 (stored as zero)."""
    assert rows % 64 == 0
    rb, c, r, b = np.ogrid[:rows // 64, :NCHUNK, :64, :64]
    col = c * 64 + b
    return np.where(col < D_IN, (rb * 64 + r) * D_IN + col, -1).astype(np.int64)


def tile_numpy(x):
    idx = tile_index(x.shape[0])
    return np.where(idx >= 0, x.reshape(-1)[np.maximum(idx, 0)], 0).astype(np.uint8)


def test_tile_index_against_brute_force():
    idx = tile_index(128)
    assert idx.shape == (2, NCHUNK, 64, 64)
    rb = 1  # one row block, not the first
    seen = set()
    for c in range(NCHUNK):
        for r in range(64):
            for b in range(64):
                col = 64 * c + b
                want = (64 * rb + r) * D_IN + col if col < D_IN else -1
                assert idx[rb, c, r, b] == want, (c, r, b)
                seen.add(want)
    # the block's real bytes, each exactly once, and the pad
    assert seen == set(range(64 * D_IN, 128 * D_IN)) | {-1}
    assert int((idx[rb] < 0).sum()) == 64 * (M.D_IN_PAD - D_IN)


@functools.lru_cache(maxsize=None)
def _shard(rows, seed):
    """Random pixels (every byte value, no structure a wrong index could hide behind) and labels;
    computed once, never modified."""
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (rows, D_IN), dtype=np.uint8), g.integers(0, M.CLASSES, rows, dtype=np.uint8)


@pytest.fixture
def rows_bm():
    from serverless_learn_amd.ops import _native

    yield lambda bm: _native.call("sl_mlp_set_rows_bm", bm)
    _native.call("sl_mlp_set_rows_bm", 0)


@gpu
@pytest.mark.parametrize("rows", [64, 128, 192, 3 * 128])
def test_relayout_is_exact(rows):
    from serverless_learn_amd.ops import _native as n

    x, _ = _shard(rows, 11)
    nbytes = int(n.lib().sl_mlp_x_tile_bytes(rows))
    assert nbytes == rows // 64 * NCHUNK * BRICK
    src = torch.from_numpy(x).cuda()
    want = tile_numpy(x)
    # every byte of dst is written: a byte left alone cannot equal `want` under both fills
    # (the issue's 0xFF, and 0x00 for the bytes that are 0xFF themselves)
    for fill in (0xFF, 0x00):
        dst = torch.full((nbytes + 256,), fill, dtype=torch.uint8, device="cuda")  # + a guard band
        n.call("sl_mlp_x_tile", n.ptr(src), n.ptr(dst), rows, n.stream_ptr())
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        tiled = got[:nbytes].reshape(want.shape)
        assert np.array_equal(tiled, want)
        assert (tiled[:, NCHUNK - 1, :, D_IN - 64 * (NCHUNK - 1):] == 0).all()  # pad columns
        assert (got[nbytes:] == fill).all()  # nothing past the end


def _trainer(batch, n_batches, cursor, **kw):
    x, y = _shard(n_batches * batch, 7)
    tr = M.FusedMLPTrainer(batch=batch, flat=M.init_params(2), **kw)
    tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
    tr.cursor.fill_(cursor)
    assert tr.xt is not None and tr.xt.numel() == n_batches * batch // 64 * NCHUNK * BRICK
    return tr


def _bits(t):
    return t.contiguous().view(torch.uint8).cpu().clone()


@gpu
@pytest.mark.parametrize("batch,bm", [(128, 128), (384, 128), (64, 64), (192, 64)])
def test_rows_kernel_tiled_equals_row_major(batch, bm, rows_bm):
    from serverless_learn_amd.ops import _native

    rows_bm(bm)
    assert _native.lib().sl_mlp_rows_bm(batch) == bm
    tr = _trainer(batch, 3, 2)
    outs = ("h1t", "dh2t", "dh1t", "w3p", "loss", "correct")

    def run():
        for k in outs:  # the same bytes under both runs, where a kernel writes nothing
            getattr(tr, k).view(torch.uint8).fill_(0x5A)
        tr._rows(True)
        torch.cuda.synchronize()
        return {k: _bits(getattr(tr, k)) for k in outs}

    assert tr._launches()["rows"].entry == "sl_mlp_rows_xt"
    tiled = run()
    tr.xt = None
    assert tr._launches()["rows"].entry == "sl_mlp_rows"
    plain = run()
    for k in outs:
        assert torch.equal(tiled[k], plain[k]), k
    # the batch under the cursor was read, not batch 0: its labels decide `correct` and the loss
    assert float(tr.loss.sum()) > 0 and not torch.equal(tiled["loss"], torch.full_like(tiled["loss"], 0x5A))


@gpu
@pytest.mark.parametrize("batch,slices", [(256, 0), (1024, 0), (1024, 3)])
def test_wgrad_tiled_equals_row_major(batch, slices):
    """Slices of one 64-row stage (the library's count for these batches) and, at (1024, 3),
    of 6, 6 and 4 stages: the ring wraps and the last slice is short."""
    from serverless_learn_amd.ops import _native

    tr = _trainer(batch, 3, 1, slices=slices or None)
    assert tr.slices == _native.lib().sl_mlp_wgrad_slices(batch, slices)
    tr._rows(True)

    def run():
        tr.slab.fill_(-7.0)
        tr._wgrad()
        torch.cuda.synchronize()
        return _bits(tr.slab)

    assert tr._launches()["wgrad"].entry == "sl_mlp_wgrad_xt"
    tiled = run()
    tr.xt = None
    assert tr._launches()["wgrad"].entry == "sl_mlp_wgrad"
    plain = run()
    assert torch.equal(tiled, plain)
    assert not torch.equal(tiled, _bits(torch.full_like(tr.slab, -7.0)))


@gpu
@pytest.mark.parametrize("graph", [False, True])
def test_trainer_tiled_equals_row_major(graph, monkeypatch):
    def train(xtile):
        if xtile:
            monkeypatch.delenv("SL_MLP_XTILE", raising=False)
        else:
            monkeypatch.setenv("SL_MLP_XTILE", "0")
        x, y = _shard(3 * 256, 7)
        tr = M.FusedMLPTrainer(batch=256, flat=M.init_params(2))
        tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
        assert (tr.xt is not None) == xtile
        if graph:
            tr.capture(warmup=2, unroll=3)  # two eager steps, then the 3-step graph twice
        tr.steps(6)
        torch.cuda.synchronize()
        assert int(tr.cursor) == (8 if graph else 6)
        return _bits(tr.params), _bits(tr.mom), _bits(tr.loss)

    a, b = train(False), train(True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
