"""Per-class weight decay on the GPU (elementwise.hip opt_flat_groups_kernel, mlp_fused.hip
GROUPS): every grouped update path against the ungrouped kernels, bit for bit.

The yardstick is the existing kernel: a grouped launch must leave, in every element, what the
ungrouped launch leaves when it runs with the decay of that element's class (no tolerance), and
with all three decays equal it must be the ungrouped run.  Only the last test compares with the
float64 reference, at the bound tests/test_optim_gpu.py test_resnet_adamw_matches_float64 uses.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from serverless_learn_amd.ops import optim as O
from serverless_learn_amd.ops.optim import CLS_BIAS, CLS_WEIGHT, DECAY_BLOCK
from serverless_learn_amd.utils import decay_exact as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
W = 0.5
RULES = {"adamw": dict(optimizer="adamw", lr=1e-3),
         "sgd": dict(lr=0.05, momentum=0.9, lr_schedule="cosine", lr_warmup_steps=2, lr_decay_steps=8)}
SHADOWS = ("w1h", "w2h", "w2th", "w3h", "w3th", "r1p")
# tests/test_optim_gpu.py's fp32 rounding bounds (derived there)
W_TOL, V_RTOL, V_FLOOR, M_TOL = 1e-6, 4e-6, 1e-30, 2.0 ** -18


# ---- 1. the flat kernels (the shipped build here; the deterministic one in section 3) ----
@pytest.mark.parametrize("case", X.flat_cases(), ids=lambda c: "n%d-%s-%s-%s-step%d" % (
    c[0], "adamw" if c[1] else "sgd", "tab" if c[2] else "lr", "bf16" if c[3] else "noshadow", c[4]))
def test_flat_groups_select_the_ungrouped_results(case):
    assert X.flat_case(DEV, *case) == []


def test_flat_groups_refuse_bad_arguments():
    n = 128
    w, g, m = (torch.zeros(n, device=DEV) for _ in range(3))
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    cls = torch.zeros(2, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="sl_sgd_flat_lr_groups"):
        O.sgd_flat_lr_groups(w, g, m, step, None, cls, (0.1, -0.1, 0.0), lr=0.1)
    with pytest.raises(AssertionError, match="shorter"):
        O.sgd_flat_lr_groups(w, g, m, step, None, cls[:1], (0.1, 0.1, 0.0), lr=0.1)


# ---- 2. the MLP engine ----
def _shard():
    from serverless_learn_amd.data.synthetic import make_mnist_like

    x, y = make_mnist_like(256, seed=3)
    return torch.from_numpy(x), torch.from_numpy(y)


class _Mlp:
    """A trainer on the shard, stepping through one of the three update forms."""

    def __init__(self, batch, form, **kw):
        from serverless_learn_amd.models.mlp import FusedMLPTrainer

        if form == "update":  # the path that clipping and accumulation steps take
            kw["clip_grad_norm"] = float("inf")
        self.tr = FusedMLPTrainer(batch=batch, device=DEV, seed=1, **kw)
        self.tr.load_shard(*_shard())
        self.ex = None
        if form == "xupdate":
            from serverless_learn_amd.parallel.xgmi import XgmiExchange

            self.ex = XgmiExchange(self.tr.n_pad, 0, 1, self.tr.device, allgather=lambda b: [b],
                                   all_ok=lambda ok: ok)
            self.tr.enable_xgmi(self.ex)

    def __enter__(self):
        return self.tr

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.tr.drop_graphs()
        if self.ex is not None:
            assert not self.ex.error()
            self.ex.close()


def _per_element():
    from serverless_learn_amd.models.mlp import N_PARAMS, CPUTrainer

    cls = CPUTrainer(batch=64, bias_weight_decay=0.0).decay_cls
    return cls.long().repeat_interleave(DECAY_BLOCK)[:N_PARAMS].to(DEV)


def _snap(tr):
    from serverless_learn_amd.models.mlp import N_PARAMS

    torch.cuda.synchronize()
    d = {k: getattr(tr, k)[:N_PARAMS].clone() for k in ("params", "mom", "v") if getattr(tr, k) is not None}
    d.update({k: getattr(tr, k).clone() for k in SHADOWS})
    d["opt_step"], d["cursor"] = tr.opt_step.clone(), tr.cursor.clone()
    return d


@pytest.mark.parametrize("form", ["sgd", "update", "xupdate"])
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("batch", [64, 128])
def test_mlp_grouped_step_composes_the_ungrouped_steps(batch, rule, form):
    """One step from the same seed and shard: weights as under W, biases as under 0."""
    snaps = []
    for kw in (dict(weight_decay=W, bias_weight_decay=0.0), dict(weight_decay=W), dict(weight_decay=0.0)):
        with _Mlp(batch, form, **kw, **RULES[rule]) as tr:
            lc = tr._launches()
            used = lc["xupdate" if form == "xupdate" else form].name
            assert used == ("sl_mlp_opt_xgmi" if form == "xupdate" else "sl_mlp_opt") + \
                ("_groups" if tr.opt.grouped else ""), used
            tr.step()
            snaps.append(_snap(tr))
    got, ref_w, ref_0 = snaps
    per = _per_element()
    for k in ("params", "mom") + (("v",) if rule == "adamw" else ()):
        assert torch.equal(got[k][per == CLS_WEIGHT], ref_w[k][per == CLS_WEIGHT]), (k, "weights")
        assert torch.equal(got[k][per == CLS_BIAS], ref_0[k][per == CLS_BIAS]), (k, "biases")
    assert not torch.equal(ref_w["params"][per == CLS_BIAS], ref_0["params"][per == CLS_BIAS])
    assert not torch.equal(ref_w["params"][per == CLS_WEIGHT], ref_0["params"][per == CLS_WEIGHT])
    for k in SHADOWS + ("opt_step", "cursor"):  # the shadows and the W1 row sums hold weights only
        assert torch.equal(got[k], ref_w[k]), k
    assert int(got["opt_step"].item()) == 1 and int(got["cursor"].item()) == 1


@pytest.mark.parametrize("rule", list(RULES))
def test_mlp_grouped_graph_replays_equal_eager_and_ungrouped(rule):
    kw = dict(weight_decay=1e-2, **RULES[rule])
    grp = dict(norm_weight_decay=1e-2, bias_weight_decay=1e-2)
    snaps = []
    for graph, extra in ((True, grp), (False, grp), (False, {})):
        with _Mlp(128, "sgd", **kw, **extra) as tr:
            if graph:
                tr.capture(warmup=0)
            for _ in range(3):
                tr.step()
            snaps.append(_snap(tr))
            assert int(tr.opt_ticket.item()) == 0
    for other, what in ((snaps[1], "graph vs eager"), (snaps[2], "grouped vs ungrouped")):
        for k, t in snaps[0].items():
            assert torch.equal(t, other[k]), (what, k)
    assert int(snaps[0]["opt_step"].item()) == 3


def test_mlp_set_optimizer_changes_the_values_not_the_switch():
    with _Mlp(64, "sgd", weight_decay=0.1, bias_weight_decay=0.0) as tr:
        assert tr.opt.grouped and tr.opt_step is not None and tr.lr_tab is None  # fixed lr: RULE_SGD_LR, scalar lr
        lc = tr._launches()
        tr.set_optimizer(bias_weight_decay=0.05)
        assert tr._launches() is not lc and tr.opt.decays() == (0.1, 0.1, 0.05)
        with pytest.raises(ValueError, match="decay groups"):
            tr.set_optimizer(bias_weight_decay=None)
    with _Mlp(64, "sgd", weight_decay=0.1) as tr:
        with pytest.raises(ValueError):
            tr.set_optimizer(bias_weight_decay=0.0)


def test_default_trainers_are_untouched():
    """An ungrouped trainer: no class map, the launches and the state keys it had."""
    for kw, names in ((dict(), {"sl_mlp_rows", "sl_mlp_wgrad", "sl_mlp_sgd"}),
                      (dict(weight_decay=0.1, **RULES["adamw"]), {"sl_mlp_rows", "sl_mlp_wgrad", "sl_mlp_sgd",
                                                                  "sl_mlp_opt"})):
        with _Mlp(64, "sgd", **kw) as tr:
            assert not hasattr(tr, "decay_cls") and not hasattr(tr, "decay_vec")
            assert {l.name for l in tr._launches().values() if not isinstance(l, list)} == names
            assert set(tr.state_extra()) == ({"cursor"} if not kw else {"cursor", "opt_step", "exp_avg_sq"})
    with _Mlp(64, "sgd", weight_decay=0.1, bias_weight_decay=0.0, **RULES["adamw"]) as tr:
        assert tr.decay_cls.is_cuda and tr.decay_cls.dtype == torch.uint8
        assert set(tr.state_extra()) == {"cursor", "opt_step", "exp_avg_sq"}  # decay is no state


# ---- 3. the ResNet engine (and the flat kernels) in the deterministic build ----
@pytest.fixture(scope="module")
def det_run():
    """scripts/decay_groups_det.py at the smallest batch the engine's tests use, in a child process
    (a process loads one kernel library)."""
    out = subprocess.run(["timeout", "-k", "10", "280", sys.executable,
                          os.path.join(ROOT, "scripts", "decay_groups_det.py"), "32", "3"],
                         env=dict(os.environ, SL_DETERMINISTIC="1"), capture_output=True, text=True, timeout=295)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["deterministic_build"], r
    return r


def test_flat_groups_in_the_deterministic_build(det_run):
    assert det_run["flat_failures"] == {}


@pytest.mark.parametrize("rule", ["adamw", "sgd"])
def test_resnet_grouped_step_composes_three_ungrouped_steps(det_run, rule):
    r = det_run[f"compose_{rule}"]
    assert r["differ"] == [] and r["refs_distinct"] and r["shadow_ok"], r
    assert r["tensors"] == (["mom", "params", "v"] if rule == "adamw" else ["mom", "params"]), r
    assert all(n > 0 for n in r["class_elements"]), r


def test_resnet_equal_decays_are_the_ungrouped_run_and_graph_equals_eager(det_run):
    r = det_run["equal_decays"]
    assert r["graph_equals_eager"] and r["grouped_equals_ungrouped"] and r["finite"], r
    assert r["opt_step"] == [4, 4, 4] and not det_run["ungrouped_has_map"], det_run


# ---- 4. the ResNet engine in the shipped build, against the CPU trainer's reference update ----
def test_resnet_grouped_adamw_matches_the_cpu_trainer():
    from serverless_learn_amd.data.synthetic import make_cifar_like
    from serverless_learn_amd.models.resnet import CPUResNetTrainer
    from serverless_learn_amd.models.resnet_engine import FusedResNetTrainer

    kw = dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2, lr_warmup_steps=2, norm_weight_decay=0.0,
              bias_weight_decay=0.0)
    x, y = make_cifar_like(2 * 32, seed=5)
    tr = FusedResNetTrainer(batch=32, device=DEV, seed=2, **kw)
    tr.load_shard(torch.from_numpy(x), torch.from_numpy(y))
    w0 = tr.get_flat().cpu()
    rec = []
    tr.allreduce = lambda g: rec.append(g.clone())
    for _ in range(3):
        tr.step()
    torch.cuda.synchronize()
    grads = [g.cpu() for g in rec]
    assert int(tr.opt_step.item()) == 3 and int(tr.cursor.item()) == 3
    # the CPU trainer's update (TrainerState._opt_update: the definition), on float64 state
    cpu = CPUResNetTrainer(batch=32, seed=2, flat=w0, **kw)
    assert torch.equal(cpu.decay_cls, tr.decay_cls.cpu())
    cpu.params, cpu.mom, cpu.v = w0.double(), torch.zeros_like(w0).double(), torch.zeros_like(w0).double()
    for g in grads:
        cpu._opt_update(g.double())
    w, m, v = tr.get_flat().cpu(), tr.mom.cpu(), tr.v.cpu()
    gmax = torch.stack([g.abs() for g in grads]).max(0).values.double()
    ew = float((w.double() - cpu.params).abs().max())
    em = (m.double() - cpu.mom).abs()
    ev = (v.double() - cpu.v).abs()
    print(f"resnet grouped adamw: max |w - w_ref| = {ew:.3e} (bound {W_TOL:.0e}); max |m - m_ref| / max_k |g_k| = "
          f"{float((em / gmax.clamp_min(1e-300)).max()):.3e} (bound {M_TOL:.3e}); max |v - v_ref| / v_ref = "
          f"{float((ev / cpu.v.clamp_min(V_FLOOR)).max()):.3e} (bound {V_RTOL:.0e})")
    assert ew <= W_TOL, ew
    assert bool((em <= M_TOL * gmax).all()), float((em - M_TOL * gmax).max())
    assert bool((ev <= V_RTOL * cpu.v + V_FLOOR).all()), float((ev / cpu.v.clamp_min(V_FLOOR)).max())
    assert torch.equal(tr.shadow, tr.params.to(torch.bfloat16))
    # the decay acted by class: the ungrouped reference from the same gradients differs on the weights only
    # where both decay, and the BatchNorm scales moved differently
    per = cpu.decay_cls.long().repeat_interleave(DECAY_BLOCK)
    un = O.OptSpec(**{k: v for k, v in kw.items() if k not in ("norm_weight_decay", "bias_weight_decay")})
    wu, mu, vu = w0.double(), torch.zeros_like(w0).double(), torch.zeros_like(w0).double()
    for k, g in enumerate(grads):
        un.update(wu, mu, vu, g.double(), k)
    assert float((wu - cpu.params)[per == CLS_WEIGHT].abs().max()) == 0.0
    assert float((wu - cpu.params)[per != CLS_WEIGHT].abs().max()) > 10 * W_TOL
