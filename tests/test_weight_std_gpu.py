"""The weight-standardization kernels (csrc/kernels/weight_std.hip) against the float64
``standardize_weight`` and autograd through it, and the ResNet engine under ``weight_std=True``."""
import functools

import pytest
import torch
import torch.nn.functional as F

from serverless_learn_amd.models.resnet import WS_EPS, ConvSpec, ref_grads, running_stats, standardize_weight
from serverless_learn_amd.ops import cnn as K
from serverless_learn_amd.ops import optim as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
# (m, k, cin, cin_real): n = 72 with 27 real columns and a partial workgroup; the ImageNet stem (392); 16 live
# lanes (64); a partial last round (576); NV classes 5 (1152) and 9 (2304); every lane for 18 rounds (4608)
CASES = [(6, 3, 8, 3), (4, 7, 8, 3), (5, 1, 64, 64), (4, 3, 64, 64), (4, 3, 128, 128), (4, 3, 256, 256),
         (3, 3, 512, 512)]
SENT, MARK = 7.0, -3.0  # what the launches must leave outside the banks, in shadow and in grad
CONST_ROW, ZERO_ROW = (0, 2), (3, 1)  # (bank, row): a constant filter (padding columns too) and an all-zero one


def _banks(cases, first=64):
    """The cases as banks of one flat vector, at 64-element boundaries with a gap of at least 64 between them."""
    out, off = [], first
    for i, (m, k, cin, real) in enumerate(cases):
        out.append(ConvSpec(f"bank{i}", cin, real, m, k, 1, 0, off))
        off += (out[-1].numel + 63) // 64 * 64 + 64
    return out, off


def _rows(t, c):
    return t[c.off:c.off + c.numel].view(c.cout, c.k, c.k, c.cin)


@functools.lru_cache(maxsize=None)
def _run():
    """Both launches, twice, over all cases in one plan: name -> CPU tensor (inputs included)."""
    banks, total = _banks(CASES)
    g = torch.Generator().manual_seed(11)
    w, grad = torch.zeros(total), torch.full((total,), MARK)
    for c in banks:
        _rows(w, c).copy_(0.05 * torch.randn(c.cout, c.k, c.k, c.cin, generator=g) + 0.1)
        _rows(grad, c).copy_(torch.randn(c.cout, c.k, c.k, c.cin, generator=g))
    _rows(w, banks[CONST_ROW[0]])[CONST_ROW[1]] = 0.1
    _rows(w, banks[ZERO_ROW[0]])[ZERO_ROW[1]] = 0.0
    o = dict(w=w, G=grad)
    plan = K.wstd_plan(banks, DEV)
    wd = w.to(DEV)
    for rep in ("", "2"):
        sh = torch.full((total,), SENT, dtype=torch.bfloat16, device=DEV)
        st, gd = torch.zeros(plan.rows, 2, device=DEV), grad.to(DEV)
        K.wstd_fwd(wd, sh, plan, stats_out=st, eps=WS_EPS)
        K.wstd_bwd(wd, gd, plan, eps=WS_EPS)
        o.update({"shadow" + rep: sh, "stats" + rep: st, "dw" + rep: gd})
    torch.cuda.synchronize()
    assert torch.equal(wd.cpu(), w)
    return banks, {k: v.cpu() for k, v in o.items()}


def _ref(c, o):
    """float64: (w, what, mu, r, G, dL/dw by autograd) of one bank."""
    w = _rows(o["w"], c).double().requires_grad_(True)
    what = standardize_weight(w, c.cin_real)
    G = _rows(o["G"], c).double()
    (dw,) = torch.autograd.grad(what, w, G)
    real = w.detach()[..., :c.cin_real]
    mu = real.mean((1, 2, 3), keepdim=True)
    r = (((real - mu) ** 2).mean((1, 2, 3), keepdim=True) + WS_EPS) ** -0.5
    return w.detach(), what.detach(), mu, r, G, dw


@pytest.mark.parametrize("i", range(len(CASES)))
def test_forward(i):
    """what is formed in fp64 and rounded to fp32, then to bf16: 2^-24 and 2^-8 of the value (2^-8 + 2^-23 covers
    their product); the fp64 chain behind it, at most 4608 + 6 additions and a few operations at 2^-53 each, is
    below 2^-40 of (|w| + |mu|) r.  The statistics are fp64 values rounded once to fp32."""
    banks, o = _run()
    c = banks[i]
    w, what, mu, r, _, _ = _ref(c, o)
    y = _rows(o["shadow"], c).double()
    bound = (2.0 ** -8 + 2.0 ** -23) * what.abs() + 2.0 ** -40 * (w.abs() + mu.abs()) * r
    assert bool(((y - what).abs() <= bound).all())
    assert bool((y[..., c.cin_real:] == 0).all())  # padding columns: exactly 0
    row0 = sum(b.cout for b in banks[:i])
    st = o["stats"][row0:row0 + c.cout].double()
    scale = w[..., :c.cin_real].abs().mean((1, 2, 3))
    assert bool(((st[:, 0] - mu.flatten()).abs() <= 2 * U * scale).all())
    assert bool(((st[:, 1] / r.flatten() - 1).abs() <= 2 * U).all())
    assert all(bool((y[row] == 0).all()) for bank, row in (CONST_ROW, ZERO_ROW) if bank == i)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_backward(i):
    """dL/dw = r (G - a - what b) is formed in fp64 and rounded once to fp32: 2^-24 of a value that is at most
    r (|G| + |a| + |what b|), 2^-23 to cover the product with the fp64 error of the value itself; the fp64 sums
    behind a and b are, as in the forward, below 2^-40 of their terms' magnitudes."""
    banks, o = _run()
    c = banks[i]
    _, what, _, r, G, dw = _ref(c, o)
    R = c.k * c.k * c.cin_real
    a = G[..., :c.cin_real].sum((1, 2, 3), keepdim=True) / R
    b = (G * what).sum((1, 2, 3), keepdim=True) / R  # (what is 0 on padding)
    bound = 2.0 ** -23 * r * (G.abs() + a.abs() + (what * b).abs())
    tot = lambda t: t.abs().sum((1, 2, 3), keepdim=True) / R  # noqa: E731
    bound += 2.0 ** -40 * r * (tot(G) + what.abs() * tot(G * what))
    got = _rows(o["dw"], c).double()
    bound[..., c.cin_real:] = 0  # padding columns: exactly 0
    assert bool(torch.isfinite(got).all()) and bool(((got - dw).abs() <= bound).all())


def test_sentinels_and_determinism():
    banks, o = _run()
    out = torch.ones(o["w"].numel(), dtype=torch.bool)
    for c in banks:
        out[c.off:c.off + c.numel] = False
    assert bool((o["shadow"][out].float() == SENT).all()) and bool((o["dw"][out] == MARK).all())
    for k in ("shadow", "stats", "dw"):
        assert torch.equal(o[k].view(torch.uint8), o[k + "2"].view(torch.uint8)), k


@pytest.mark.parametrize("bank", [ConvSpec("n4612", 4612, 4612, 1, 1, 1, 0, 64), ConvSpec("n6", 6, 6, 2, 1, 1, 0, 64),
                                  ConvSpec("off66", 64, 64, 2, 1, 1, 0, 66)], ids=lambda c: c.name)
def test_unsupported_banks_are_refused_and_write_nothing(bank):
    plan = K.wstd_plan([bank], DEV)
    w = torch.ones(8192, device=DEV)
    sh, g = torch.full((8192,), SENT, dtype=torch.bfloat16, device=DEV), torch.full((8192,), MARK, device=DEV)
    with pytest.raises(RuntimeError):
        K.wstd_fwd(w, sh, plan)
    with pytest.raises(RuntimeError):
        K.wstd_bwd(w, g, plan)
    torch.cuda.synchronize()
    assert bool((sh.float() == SENT).all()) and bool((g == MARK).all())


def _trainer(norm="batch", **kw):
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    tr = FusedResNetTrainer(batch=32, device=DEV, momentum=0.0, weight_decay=0.0, norm=norm, **kw)
    x, y = (torch.from_numpy(a) for a in make_cifar_like(32, seed=3))
    tr.load_shard(x, y)
    return tr, x, y


@pytest.mark.parametrize("norm", ["batch", "group"])
def test_engine_grads_match_reference(norm, monkeypatch):
    """The measures and bounds of test_cnn_gpu.py's test_resnet_engine_grads_match_reference, and the two
    projections that every standardized filter's gradient satisfies whatever the convolutions' noise: dL/dw is an
    fp64 value v rounded once to fp32 with sum_real v = 0 and sum v (w - mu) = WS_EPS r^3 sum G (w - mu) (0 but
    for WS_EPS: 1 - var r^2 = WS_EPS r^2) up to the fp64 chain, so both sums of g are within 2^-24 of the sum of
    their terms' magnitudes; c = 2 leaves the chain its share.  G is what compute_grads hands to wstd_bwd."""
    tr, x, y = _trainer(norm, weight_std=True)
    assert tr.model_name == "resnet18-cifar" + ("-gn32" if norm == "group" else "") + "-ws"
    seen, wstd_bwd = [], tr.K.wstd_bwd
    monkeypatch.setattr(tr.K, "wstd_bwd", lambda p, g, *a, **k: (seen.append(g.clone()), wstd_bwd(p, g, *a, **k)))
    g = tr.compute_grads().clone()
    assert len(seen) == 1
    kw = dict(norm="group", groups=32) if norm == "group" else {}
    loss_ref, _, g_ref = ref_grads(tr.spec, tr.params.detach().clone(), x.to(DEV), y.to(DEV), 1.0 / 32,
                                   running_stats(tr.spec, DEV), weight_std=True, **kw)
    loss = float(tr.loss.sum())
    spec, fc = tr.spec, slice(tr.spec.fc_w, tr.spec.fc_w + 5120)
    cos = {c.name: float(F.cosine_similarity(g[c.off:c.off + c.numel], g_ref[c.off:c.off + c.numel], dim=0))
           for c in spec.convs()}
    for b in spec.bns():
        idx = torch.cat([torch.arange(o, o + b.c) for o in (b.g_off, b.b_off)]).to(DEV)
        cos[b.name] = float(F.cosine_similarity(g[idx], g_ref[idx], dim=0))
    cos["fc"] = float(F.cosine_similarity(g[fc], g_ref[fc], dim=0))
    print(norm, "loss", loss, float(loss_ref), "cosines", {k: round(v, 4) for k, v in cos.items()})
    assert abs(loss - float(loss_ref)) / float(loss_ref) < 0.03, (loss, float(loss_ref))
    assert cos.pop("fc") > 0.99
    assert not {k: v for k, v in cos.items() if v < 0.85}
    for c in spec.convs():
        gr, G, w = (_rows(t, c).double().cpu() for t in (g, seen[0], tr.params))
        assert bool((gr[..., c.cin_real:] == 0).all())
        gr, G, w = (t[..., :c.cin_real] for t in (gr, G, w))
        d = w - w.mean((1, 2, 3), keepdim=True)
        rest = WS_EPS * ((d * d).mean((1, 2, 3)) + WS_EPS) ** -1.5 * (G * d).sum((1, 2, 3))
        for q, want in ((gr, 0.0), (gr * d, rest)):
            assert bool(((q.sum((1, 2, 3)) - want).abs() <= 2 * U * q.abs().sum((1, 2, 3))).all()), c.name


@pytest.mark.parametrize("norm", ["batch", "group"])
def test_engine_shadow_is_the_standardized_weights(norm):
    """After eager steps, after captured replays and after evaluate(ema=True)'s swap: the whole shadow is
    bf16(params) with wstd_fwd over the conv banks, so the fc slice is bf16(params)."""
    tr, x, y = _trainer(norm, weight_std=True, ema_decay=0.9)

    def check():
        want = torch.empty_like(tr.shadow)
        O.to_bf16(tr.params, want)
        K.wstd_fwd(tr.params, want, tr.wstd, eps=WS_EPS)
        torch.cuda.synchronize()
        assert torch.equal(tr.shadow.view(torch.int16), want.view(torch.int16))
        assert bool(torch.isfinite(tr.params).all())
        fc = slice(tr.spec.fc_w, tr.spec.fc_w + 5120)
        assert torch.equal(tr.shadow[fc], tr.params[fc].bfloat16())

    for _ in range(2):
        tr.step()
    check()
    tr.evaluate(x, y, ema=True)
    check()
    tr.capture(warmup=1)
    for _ in range(2):
        tr.step()
    check()
    assert int(tr.cursor.item()) == 5 and tr.graph is not None
    tr.drop_graphs()


def test_default_trainer_launches_neither_kernel(monkeypatch):
    tr, _, _ = _trainer()

    def boom(*a, **k):
        raise AssertionError("a weight-standardization kernel launched by a default trainer")

    monkeypatch.setattr(tr.K, "wstd_fwd", boom)
    monkeypatch.setattr(tr.K, "wstd_bwd", boom)
    tr.step()
    tr.compute_grads()
    tr.refresh_shadows()
    torch.cuda.synchronize()
    assert tr.wstd is None and not tr.weight_std and tr.model_name == "resnet18-cifar"
