"""The per-sample GroupNorm kernels (csrc/kernels/groupnorm.hip) against float64 references, their
bit-for-bit determinism in and across the two builds, and the ResNet engine under norm="group".
What compares bits between builds or between runs of a step is computed by one SL_DETERMINISTIC=1
child process (this file's ``__main__``), as in tests/test_classes_gpu.py."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from serverless_learn_amd.ops import cnn as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
# (N, H, C, G): cpg 1 on a tiny slab with odd N; cpg 64 on eight slabs; two slabs; the full 128 KB
# slab (32 rows per thread); 8 rows per thread
CASES = [(3, 4, 64, 64), (3, 4, 512, 8), (2, 8, 128, 32), (2, 32, 64, 8), (2, 16, 256, 16)]
MASKS = ("ymask", "recompute", "none")
# The chain of additions behind a statistic, read off slab_reduce and slab_stats, is 32 rows of a thread, 3 xor
# shuffles, 3 waves and 63 channels of a group, all in fp64 (2^-53 each); fp32 enters once, where the result is stored.
L_STAT = 1 + (32 + 3 + 3 + 63) * 2.0 ** -29


@functools.lru_cache(maxsize=None)
def _run(case):
    """Every variant of the three kernels on one seeded input: name -> tensor (inputs included)."""
    N, H, C, G = case
    g = torch.Generator().manual_seed(sum(case))
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    o = dict(x=(rn(N, H, H, C) * 1.5 + 0.75).bfloat16(), res=rn(N, H, H, C).bfloat16(), dy=rn(N, H, H, C).bfloat16(),
             gamma=1 + 0.5 * rn(C), beta=0.3 * rn(C))
    o = {k: v.to(DEV) for k, v in o.items()}
    x, mean, rstd = o["x"], torch.empty(N, G, device=DEV), torch.empty(N, G, device=DEV)
    for r, relu in ((0, 0), (0, 1), (1, 0), (1, 1)):
        y = torch.empty_like(x)
        m = torch.empty(x.numel() // 8, dtype=torch.uint8, device=DEV) if relu else None
        K.gn_fwd(x, o["gamma"], o["beta"], y, mean, rstd, G, relu=bool(relu), res=o["res"] if r else None, mask_out=m)
        o[f"y{r}{relu}"], o[f"m{r}{relu}"] = y, m
    o["mean"], o["rstd"] = mean, rstd
    ws = torch.empty(K.gn_ws_floats(N, C), device=DEV)
    for src in MASKS:
        dx, gg, gb = torch.empty_like(x), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dz = torch.empty_like(x) if src == "ymask" else None
        K.gn_bwd(o["dy"], x, o["gamma"], o["beta"], mean, rstd, dx, ws, G, dz_out=dz,
                 y_mask=o["m11"] if src == "ymask" else None, recompute_mask=src == "recompute")
        K.gn_param_fold(ws, N, gg, gb)
        o.update({"dx_" + src: dx, "dz_" + src: dz, "gg_" + src: gg, "gb_" + src: gb})
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items() if v is not None}


def _digest(o):
    return {k: hashlib.sha256(v.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() for k, v in o.items()}


def _grouped(t, case):
    N, H, C, G = case
    return t.double().view(N, H * H, G, C // G)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("res", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_forward(case, res, relu):
    o, (N, H, C, G) = _run(case), case
    xg = _grouped(o["x"], case)
    mean = xg.mean((1, 3), keepdim=True)
    rstd = (((xg - mean) ** 2).mean((1, 3), keepdim=True) + 1e-5) ** -0.5
    scale = xg.abs().mean((1, 3))
    e_mean = ((o["mean"].double() - mean[:, 0, :, 0]).abs() / scale).max()
    e_rstd = (o["rstd"].double() / rstd[:, 0, :, 0] - 1).abs().max()
    norm = ((xg - mean) * rstd).view(o["x"].shape) * o["gamma"].double() + o["beta"].double()
    r = o["res"].double() if res else torch.zeros_like(norm)
    ref = norm + r
    ref = ref.clamp(min=0) if relu else ref
    y = o[f"y{res}{relu}"]
    over = (y.double() - ref).abs() - (2.0 ** -8 * ref.abs() + 2.0 ** -20 * (norm.abs() + r.abs()))
    slack = over.max()
    print(case, res, relu, "mean, rstd err / u", float(e_mean) / U, float(e_rstd) / U, "y excess", float(slack),
          "elements over", int((over > 0).sum()), "of", over.numel(), "|ref| there", float(ref.abs().flatten()[over.argmax()]))
    assert float(e_mean) <= L_STAT * U and float(e_rstd) <= L_STAT * U and float(slack) <= 0
    if relu:
        assert torch.equal(((o[f"m{res}{relu}"][:, None] >> torch.arange(8)) & 1).bool().view(y.shape), y > 0)


@pytest.mark.parametrize("src", MASKS)
@pytest.mark.parametrize("case", CASES)
def test_backward(case, src):
    o, (N, H, C, G) = _run(case), case
    m = H * H * C // G
    mask = {"ymask": o["y11"] > 0, "recompute": o["y01"] > 0, "none": torch.ones_like(o["x"], dtype=torch.bool)}[src]
    dz = o["dy"] * mask
    if src == "ymask":
        assert torch.equal(o["dz_ymask"], dz)
    bc = lambda t: t.double()[:, None, :, None]  # noqa: E731  ([N, G] over the grouped view)
    xh = (_grouped(o["x"], case) - bc(o["mean"])) * bc(o["rstd"])
    gdz = _grouped(dz.double() * o["gamma"].double(), case)
    t1, t2, t3 = gdz, gdz.sum((1, 3), keepdim=True) / m, xh * (gdz * xh).sum((1, 3), keepdim=True) / m
    ref = (bc(o["rstd"]) * (t1 - t2 - t3)).view(dz.shape)
    terms = (bc(o["rstd"]) * (t1.abs() + t2.abs() + t3.abs())).view(dz.shape)
    slack = ((o["dx_" + src].double() - ref).abs() - (2.0 ** -8 * ref.abs() + 2.0 ** -18 * terms)).max()
    # L': slab_reduce's 32 + 3 + 3 per-channel additions, N - 1 of the fold, 1 into the gradient, and the 3
    # roundings of dz * ((x - mean) * rstd)
    lp = 32 + 3 + 3 + N + 3
    pg = dz.double() * xh.view(dz.shape)
    e_g = ((o["gg_" + src].double() - pg.sum((0, 1, 2))).abs() - lp * U * pg.abs().sum((0, 1, 2))).max()
    e_b = ((o["gb_" + src].double() - dz.double().sum((0, 1, 2))).abs() - lp * U * dz.double().abs().sum((0, 1, 2))).max()
    assert float(slack) <= 0 and float(e_g) <= 0 and float(e_b) <= 0


@pytest.mark.parametrize("hw_c_g", [(33 * 32, 64, 8), (16, 128, 1), (16, 96, 8)])
def test_unsupported_shapes_are_refused_and_write_nothing(hw_c_g):
    hw, c, g = hw_c_g
    x, ga = torch.ones(1, hw, 1, c, dtype=torch.bfloat16, device=DEV), torch.ones(c, device=DEV)
    y, st = torch.full_like(x, 7.0), torch.full((2, 1, g), 7.0, device=DEV)
    with pytest.raises(RuntimeError):
        K.gn_fwd(x, ga, ga, y, st[0], st[1], g)
    with pytest.raises(RuntimeError):
        K.gn_bwd(x, x, ga, ga, st[0], st[1], y, torch.empty(2 * c, device=DEV), g)
    torch.cuda.synchronize()
    assert bool((y == 7).all()) and bool((st == 7).all())


@pytest.fixture(scope="module")
def det_child():
    env = dict(os.environ, SL_DETERMINISTIC="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=280)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["deterministic_build"], r
    return r


@pytest.mark.parametrize("case", CASES)
def test_same_bits_twice_and_in_both_builds(case, det_child):
    first = _digest(_run(case))
    assert _digest(_run.__wrapped__(case)) == first and det_child["digests"][str(case)] == first


def _trainer(groups, **kw):
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    tr = FusedResNetTrainer(batch=32, device=DEV, momentum=0.0, weight_decay=0.0, norm="group", norm_groups=groups, **kw)
    x, y = (torch.from_numpy(a) for a in make_cifar_like(32, seed=3))
    tr.load_shard(x, y)
    return tr, x, y


@pytest.mark.parametrize("groups", [8, 32])
def test_engine_grads_match_reference(groups):
    """The measures and bounds of test_cnn_gpu.py's test_resnet_engine_grads_match_reference."""
    from serverless_learn_amd.models.resnet import ref_grads

    tr, x, y = _trainer(groups)
    g = tr.compute_grads().clone()
    loss, correct = float(tr.loss.sum()), float(tr.correct.sum())
    loss_ref, _, g_ref = ref_grads(tr.spec, tr.params.detach().clone(), x.to(DEV), y.to(DEV), 1.0 / 32,
                                   norm="group", groups=groups)
    assert abs(loss - float(loss_ref)) / float(loss_ref) < 0.03, (loss, float(loss_ref))
    spec, fc = tr.spec, slice(tr.spec.fc_w, tr.spec.fc_w + 5120)
    cos = {c.name: float(F.cosine_similarity(g[c.off:c.off + c.numel], g_ref[c.off:c.off + c.numel], dim=0))
           for c in spec.convs()}
    for b in spec.bns():
        idx = torch.cat([torch.arange(o, o + b.c) for o in (b.g_off, b.b_off)]).to(DEV)
        cos[b.name] = float(F.cosine_similarity(g[idx], g_ref[idx], dim=0))
    assert float(F.cosine_similarity(g[fc], g_ref[fc], dim=0)) > 0.99
    assert not {k: v for k, v in cos.items() if v < 0.85}
    # no eval mode: evaluation is the training forward, bit for bit; and nothing beside the flat vector
    ev = tr.evaluate(x, y)
    assert (ev.loss, ev.accuracy) == (loss / 32, correct / 32)
    assert tr.running_stats() == {} and tr.buffers() == [] and tr.model_name == f"resnet18-cifar-gn{groups}"


def test_captured_step_replays_the_eager_step_and_batchnorm_is_as_it_was(det_child):
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    assert det_child["graph"] == {"captured": True, "changed_vs_eager": [], "cursor": 5, "finite": True}
    tr = FusedResNetTrainer(batch=8, device=DEV)
    assert tr.norm == "batch" and not hasattr(tr, "gn") and not hasattr(tr, "gn_ws") and "sc" not in tr.blocks[2]
    assert len(tr.running_stats()) == 20 and tr.model_name == "resnet18-cifar"


def _child():
    """SL_DETERMINISTIC=1: the kernels' digests, and two eager + three replayed steps against five eager."""
    out = {"deterministic_build": K.deterministic(), "digests": {str(c): _digest(_run(c)) for c in CASES}}
    a, b = _trainer(32, accum_steps=2)[0], _trainer(32, accum_steps=2)[0]
    a.capture(warmup=2)
    for _ in range(3):
        a.step()
    for _ in range(5):
        b.step()
    torch.cuda.synchronize()
    out["graph"] = {"captured": a.graph is not None and b.graph is None, "cursor": int(a.cursor.item()) // 2,
                    "changed_vs_eager": [k for k in ("params", "shadow", "grad", "loss") if not
                                         torch.equal(getattr(a, k), getattr(b, k))],
                    "finite": bool(torch.isfinite(a.params).all())}
    a.drop_graphs()
    print(json.dumps(out))


if __name__ == "__main__":  # the child process of det_child
    _child()
