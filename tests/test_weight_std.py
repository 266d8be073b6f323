"""weight_std=True on the CPU: the reference trainer, the invariance that defines the feature, the closed-form
backward against autograd, the Config flag and the refusals."""
import argparse

import pytest
import torch
import torch.nn.functional as F

from serverless_learn_amd.config import Config, add_cli_args, from_args
from serverless_learn_amd.models import resnet as R

HW = 8
GN = dict(norm="group", groups=8)


def _setup(n=4):
    g = torch.Generator().manual_seed(3)  # (make_cifar_like's prototypes need more than 8 x 8)
    x = torch.randint(0, 256, (n, HW, HW, 3), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (n,), generator=g, dtype=torch.uint8)
    spec = R.resnet18_spec("cifar", 10, HW)
    return spec, R.init_params(spec, 5), x, y


def test_cpu_trainer_steps_and_is_named():
    _, _, x, y = _setup()
    tr = R.CPUResNetTrainer(batch=4, in_hw=HW, norm="group", norm_groups=8, weight_std=True, lr=0.05)
    tr.load_shard(x, y)
    w0 = tr.params.clone()
    tr.step()
    assert tr.model_name == "resnet18-cifar-gn8-ws" and bool(torch.isfinite(tr.params).all())
    assert not torch.equal(tr.params, w0) and R.CPUResNetTrainer(batch=4).model_name == "resnet18-cifar"
    assert R.CPUResNetTrainer(batch=4, weight_std=True).model_name == "resnet18-cifar-ws"


@pytest.mark.parametrize("name", ["stem", "layer2.0.conv1", "layer3.0.down"])
def test_logits_ignore_a_filters_shift_and_scale(name):
    """A filter replaced by 2 w + 0.3 standardizes to the same what but for WS_EPS (its variance, at least
    2 / (9 * 512) at init, grows fourfold: r changes by less than 1e-6 / (2 * 4e-4) of itself) and fp32 rounding:
    far below 1e-3 of the logits, which the same change moves by much more without standardization."""
    spec, w, x, _ = _setup()
    c = next(c for c in spec.convs() if c.name == name)
    w2 = w.clone()
    row = w2[c.off:c.off + c.kdim]
    row.copy_(2 * row + 0.3)
    with torch.no_grad():
        on, off = (tuple(R.ref_forward(spec, v, x, weight_std=ws, **GN) for v in (w, w2)) for ws in (True, False))
    assert float((on[0] - on[1]).abs().max()) < 1e-3 * float(on[0].abs().max())
    assert float((off[0] - off[1]).abs().max()) > 1e-2 * float(off[0].abs().max())


def test_gradient_is_the_closed_form_and_its_rows_are_projected():
    """dL/dw by fp32 autograd against r (G - a - what b) in float64, G = dL/dwhat read off the same graph (the
    standardized banks written into a copy of the flat vector).  Each element passes under 16 fp32 roundings and
    two reductions of at most 4608 terms (blocked pairwise, under 16 more, relative to the sum of their terms'
    magnitudes): c = 32 on r (|G| + mean |G| + |what| mean |G what|).  The two projections hold to that bound summed over the row: sum_real g = 0, and sum g (w - mu) =
    WS_EPS r^3 sum G (w - mu), which is 0 but for WS_EPS (1 - var r^2 = WS_EPS r^2)."""
    spec, w0, x, y = _setup()
    w = w0.clone().requires_grad_(True)
    rows = lambda t, c: t[c.off:c.off + c.numel].view(c.cout, c.k, c.k, c.cin)  # noqa: E731
    flat, whats = w.clone(), {}
    for c in spec.convs():
        whats[c.name] = R.standardize_weight(rows(w, c), c.cin_real)
        whats[c.name].retain_grad()
        flat[c.off:c.off + c.numel] = whats[c.name].reshape(-1)
    (F.cross_entropy(R.ref_forward(spec, flat, x, **GN), y.long(), reduction="sum") * 0.25).backward()
    g = w.grad.double()
    for c in spec.convs():
        real = rows(w0, c).double()[..., :c.cin_real]
        mu = real.mean((1, 2, 3), keepdim=True)
        r = (((real - mu) ** 2).mean((1, 2, 3), keepdim=True) + R.WS_EPS) ** -0.5
        what, Gr, gr = (real - mu) * r, whats[c.name].grad.double()[..., :c.cin_real], rows(g, c)
        a, b = Gr.mean((1, 2, 3), keepdim=True), (Gr * what).mean((1, 2, 3), keepdim=True)
        bound = 32 * 2.0 ** -24 * r * (Gr.abs() + Gr.abs().mean((1, 2, 3), keepdim=True)
                                       + what.abs() * (Gr * what).abs().mean((1, 2, 3), keepdim=True))
        assert bool((gr[..., c.cin_real:] == 0).all()), c.name
        gr = gr[..., :c.cin_real]
        assert bool(((gr - r * (Gr - a - what * b)).abs() <= bound).all()), c.name
        assert bool((gr.sum((1, 2, 3)).abs() <= bound.sum((1, 2, 3))).all()), c.name
        rest = R.WS_EPS * r ** 3 * (Gr * (real - mu)).sum((1, 2, 3), keepdim=True)
        assert bool((((gr * (real - mu)).sum((1, 2, 3), keepdim=True) - rest).abs()
                     <= (bound * (real - mu).abs()).sum((1, 2, 3), keepdim=True)).all()), c.name
    # ref_grads(weight_std=True) is that graph: the same operations on the same values
    torch.testing.assert_close(R.ref_grads(spec, w0, x, y, 0.25, None, weight_std=True, **GN)[2].double(), g,
                               rtol=1e-4, atol=1e-7)


def test_flag_env_and_refusals(monkeypatch):
    ap = argparse.ArgumentParser()
    add_cli_args(ap)
    assert from_args(ap.parse_args(["--model", "resnet18", "--weight-std", "1"])).weight_std is True
    monkeypatch.setenv("SL_MODEL", "resnet18")
    monkeypatch.setenv("SL_WEIGHT_STD", "1")
    assert Config.from_env().weight_std is True and Config().weight_std is False
    for model in ("mlp", "simulate"):
        with pytest.raises(ValueError):
            Config(model=model, weight_std=True)
