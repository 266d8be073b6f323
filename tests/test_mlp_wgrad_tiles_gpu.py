"""The weight gradient's wide dW1 tiles (128 dH1 columns x 256 X columns, 4-slot ring) against the
256 x 128 loop they replace, and both against the float64 reference.

The wide loop keeps the instruction, the stage order and the k order of every dW1 element's sum, and
stores each accumulator where the 256 x 128 loop's wave stored it: the whole slab -- every tile,
the never-written tail columns and padding included -- must be the same BYTES with the launcher's
switch (sl_mlp_set_wg_wide) on and off.  The operands are the exact ones of
serverless_learn_amd/utils/mlp_exact.py, so the reduced gradient must also EQUAL the float64
reference, element for element, in both forms.  Shapes: the stage counts around the ring depth
(3 stages in flight, 4 slots) and a short last slice; both X layouts; the cursor on batch 2 of a
3-batch shard (reached as cursor 5, so the modulo is in it too)."""
from dataclasses import dataclass

import pytest
import torch

from serverless_learn_amd.models import mlp as M
from serverless_learn_amd.utils import mlp_exact as X

pytestmark = pytest.mark.gpu

TL_TILE = 256 * 128
SENTINEL = 0x7FC12345  # a NaN no kernel produces


@dataclass(frozen=True)
class WCase(X.Case):
    """A case outside the exact table: its own seed (the table's is the case's place in it)."""

    @property
    def seed(self) -> int:
        return 500 + self.batch + 7 * self.slices[0][1]


def _case(batch, req, eff, why):
    return WCase("W%d_%d" % (batch, eff), batch, 128 if batch % 128 == 0 else 64, ((req, eff),), shard=3 * batch,
                 cursor=5, why=why)


# (batch, requested slices, effective slices, stages per slice)
SHAPES = [
    _case(64, 1, 1, "one stage: the ring is never full"),
    _case(192, 1, 1, "three stages: exactly the in-flight depth, no refill"),
    _case(256, 1, 1, "four stages: one refill, every slot used once"),
    _case(320, 1, 1, "five stages: the ring wraps, odd stage count"),
    _case(320, 3, 3, "2 + 2 + 1 stages: short last slice"),
    _case(1024, 3, 3, "6 + 6 + 4 stages: the ring wraps twice, short last slice"),
]


def _slab_bits(case, xt, wide):
    """Rows, then the weight gradient into a sentinel-filled slab with the switch at ``wide``;
    returns the slab's bits (int32, on the CPU) and the reduced gradient."""
    from serverless_learn_amd.ops import _native

    with X._Setup(case, xt):
        tr = X._trainer(case, slices=case.slices[0][0])
        assert tr.slices == case.slices[0][1] and (tr.xt is not None) == xt
        lc = tr._launches()
        assert lc["wgrad"].entry == ("sl_mlp_wgrad_xt" if xt else "sl_mlp_wgrad")
        lc["rows"]()
        tr.slab.view(torch.int32).fill_(SENTINEL)
        _native.call("sl_mlp_set_wg_wide", 1 if wide else 0)
        try:
            lc["wgrad"]()
        finally:
            _native.call("sl_mlp_set_wg_wide", 1)
        torch.cuda.synchronize()
        bits = tr.slab.view(torch.int32).cpu().clone()
        tr.grad.fill_(float("nan"))
        lc["reduce"]()
        torch.cuda.synchronize()
        return bits, tr.grad[:M.N_PARAMS].cpu()


@pytest.mark.parametrize("layout", ["xt", "rowmajor"])
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: c.name)
def test_wide_tiles_write_the_same_slab(case, layout):
    xt = layout == "xt"
    ref = X.reference(case)
    X.check_case_bounds(case, ref)
    total = case.batch // 64
    spp = -(-total // case.slices[0][1])
    assert [min(spp, total - s * spp) for s in range(case.slices[0][1])] == {
        "W64_1": [1], "W192_1": [3], "W256_1": [4], "W320_1": [5], "W320_3": [2, 2, 1], "W1024_3": [6, 6, 4]}[case.name]
    wide, g_wide = _slab_bits(case, xt, True)
    narrow, g_narrow = _slab_bits(case, xt, False)
    # the whole slab, byte for byte (dW1 tiles, the tail tile, dW2, the db1 / db2 / dW3 bands, padding)
    if not torch.equal(wide, narrow):
        bad = (wide != narrow).nonzero()
        s, off = int(bad[0, 0]), int(bad[0, 1])
        tile, within = divmod(off, TL_TILE)
        raise AssertionError("%d slab words differ; first in slice %d tile %d wave %d store %d lane %d word %d" % (
            bad.shape[0], s, tile, within // 4096, within % 4096 // 256, within % 256 // 4, within % 4))
    # dW1's tail tile (tile 6): only its 16 real columns are written -- waves 0 and 1 (n-block 0 of
    # the two m-halves), store instructions (i, j = 0); columns 784 and above keep the sentinel
    tail = wide[:, 6 * TL_TILE:7 * TL_TILE].view(-1, 8, 8, 2, 256)  # [slice][wave][i][j][lane, word]
    written = torch.zeros(8, 8, 2, dtype=torch.bool)
    written[:2, :, 0] = True
    assert bool((tail[:, ~written] == SENTINEL).all()), "columns >= 784 of the tail tile were written"
    assert bool((tail[:, written] != SENTINEL).all()), "real columns of the tail tile were not written"
    # every word of the six full dW1 tiles and the two dW2 tiles is written
    assert bool((wide[:, :6 * TL_TILE] != SENTINEL).all()) and bool((wide[:, 7 * TL_TILE:9 * TL_TILE] != SENTINEL).all())
    # the bands [dW3 | db3 | pad | db1 | db2] behind the tiles (equal to the 256 x 128 loop's by the
    # comparison above) and every tile, through the reduce: the float64 reference, exactly
    for what, g in (("wide", g_wide), ("256 x 128 loop", g_narrow)):
        fails = X.compare_flat(g, ref["grad"], "grad (%s)" % what)
        assert not fails, "\n".join(str(m) for m in fails)
