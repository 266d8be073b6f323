"""Exact, element-wise checks of the convolution kernels (csrc/kernels/conv.hip, conv3x3_halo.hip).

The operands are small INTEGERS stored as bf16 (x, dy, add in [-2, 2], w in {-1, 0, 1}, thinned by
a density mask).  Every product and every fp32 partial sum is then an integer far below 2^24, so
the result is the same bits whatever the order of the MFMAs, split-K atomics, slab reduces, rsum
replicas or the deterministic build's fixed-point sums; and with every bf16 output kept at
|value| <= 256 every stored value is representable, so no rounding point matters.  A kernel's output
must therefore EQUAL a float64 reference, element for element: the tests use ``torch.equal`` and no
tolerance.  The magnitude bounds are conditions on the inputs, asserted on the reference
(:func:`check_bounds`) before any kernel output is looked at.

This module holds the reference (:func:`reference`, float64, tap by tap from the definition, no
convolution library), the operand generator (:func:`operands`), the case table (:data:`CASES`), the
comparator (:func:`compare`, which decodes where a mismatch sits: pixel, GEMM row, tile, parity
class) and the driver that runs one case through the launchers (:func:`run_case`).  Everything but
:func:`run_case` runs on the CPU.  Used by tests/test_conv_exact.py, tests/test_conv_exact_gpu.py
and scripts/conv_exact_check.py.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

BF16_EXACT = 256.0       # integers up to 2^8 are bf16 values (8 significand bits)
F32_EXACT = float(2 ** 24)  # integers below 2^24 are fp32 values, and so is every partial sum of them


# ---------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One convolution shape and the kernel families (ops.cnn.KERNEL_FAMILIES) it is there for.

    shape = (N, H, W, C, cout, k, stride, pad).  fwd / dgrad / wgrad: families the forward, the
    data gradient and the weight gradient must have launched.  halo / s2: the direct 3x3 path
    and the class-fused stride-2 data-gradient kernel switched on (the default) or off.
    smallm: the families instead expected under SL_GEMM_SMALLM=1 (fwd, dgrad)."""
    name: str
    shape: tuple
    fwd: tuple = ()
    dgrad: tuple = ()
    wgrad: tuple = ()
    halo: bool = True
    s2: bool = True
    do_dgrad: bool = True
    yf: bool = True            # also ask for the fp32 output (the direct kernel has none)
    even: bool = False         # also the even-position shortcut gradient + add_even
    bias: bool = False         # also a forward with a per-channel bias
    smallm: tuple = ()
    target_wgs: tuple = (2, 100, 384)   # split-K targets: slices == 1, a slice tail, the default
    ldd: int = 0               # > 0: the channel stride of dy in both gradients (the engine's dlogits stride)

    @property
    def group(self) -> str:
        return self.name[0]

    def out_hw(self):
        n, h, w, c, cout, k, s, p = self.shape
        return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1

    def rows(self) -> int:
        """GEMM rows of the forward (output pixels)."""
        oh, ow = self.out_hw()
        return self.shape[0] * oh * ow

    def density(self) -> float:
        """1/4 up to ~65,536 GEMM rows in either direction, 1/8 above (262,144-row data
        gradients).  With x uniform on [-2, 2] and w on {-1, 0, 1}, each thinned to density d,
        Var y = K d^2 4/3: 96 at K = 1152, d = 1/4, so max |y| ~ 5 sigma ~ 50 and
        sum(y^2) / M ~ 100 < 2^24 / 67,032 = 250; at d = 1/8 a quarter of that."""
        n, h, w = self.shape[:3]
        return 0.25 if max(self.rows(), n * h * w) <= 70000 else 0.125

    def macs(self) -> int:
        n, h, w, c, cout, k, s, p = self.shape
        return self.rows() * k * k * c * cout

    def cpu_sized(self) -> bool:
        """Small enough for the float64 reference on the CPU (the non-GPU tests)."""
        return self.macs() <= 5e8


def _c(name, shape, **kw):
    return Case(name, tuple(shape), **kw)


CASES = [
    # A: conv_gemm_kernel 64/128 x 64/128, row and column tails, non-uniform-tap staging
    _c("A1-3x7x7-128-256", (3, 7, 7, 128, 256, 3, 1, 1), fwd=("gemm_64x128",), dgrad=("gemm_t_64x128",),
       wgrad=("wgrad_128",), smallm=(("gemm_128x128",), ("gemm_t_128x128",))),
    _c("A2-2x5x9-64-64-nonsquare", (2, 5, 9, 64, 64, 3, 1, 1), fwd=("gemm_64x64",), dgrad=("gemm_t_64x64",),
       wgrad=("wgrad_64",), smallm=(("gemm_128x64",), ("gemm_t_128x64",))),
    _c("A3-1x6x10-64-72-1x1", (1, 6, 10, 64, 72, 1, 1, 0), fwd=("gemm_64x128",), dgrad=("gemm_t_64x64",),
       wgrad=("wgrad_128",), smallm=(("gemm_128x128",), ("gemm_t_128x64",))),
    _c("A4-fc-8x512-10", (8, 1, 1, 512, 10, 1, 1, 0), fwd=("gemm_64x64",), wgrad=("wgrad_64",), do_dgrad=False, bias=True,
       smallm=(("gemm_128x64",), ())),
    _c("A5-stem-7x7s2", (2, 20, 20, 8, 64, 7, 2, 3), fwd=("gemm_64x64",), dgrad=("gemm_t_64x64",),
       wgrad=("wgrad_64",), smallm=(("gemm_128x64",), ("gemm_t_128x64",))),
    _c("A6-cifar-stem-gemm", (4, 32, 32, 8, 64, 3, 1, 1), halo=False, fwd=("gemm_64x64",),
       dgrad=("gemm_t_64x64",), wgrad=("wgrad_64_lean",), smallm=(("gemm_128x64",), ("gemm_t_128x64",))),
    # 512 tiles of 128 rows (N = 256; at N = 128 there are 256 and the planner takes 64-row tiles)
    _c("A7-256x16x16-64-64", (256, 16, 16, 64, 64, 3, 1, 1), fwd=("gemm_128x64",), dgrad=("gemm_t_128x64",),
       wgrad=("wgrad_64_lean",)),
    # B: conv_gemm_big_kernel, forward and stride-1 transposed data gradient
    _c("B1-256x16x16-128-128", (256, 16, 16, 128, 128, 3, 1, 1), fwd=("big",), dgrad=("big_t",),
       wgrad=("wgrad_128_lean",)),
    # M = 67,032: 262 tiles, the last one 216 rows, division decode
    _c("B2-342x14x14-128-128", (342, 14, 14, 128, 128, 3, 1, 1), fwd=("big",), dgrad=("big_t",),
       wgrad=("wgrad_128",)),
    # C: conv_gemm_wide_kernel (>= 512 tiles of 256 x 128)
    _c("C1-256x16x16-64-256", (256, 16, 16, 64, 256, 3, 1, 1), fwd=("wide",), dgrad=("gemm_t_128x64",),
       wgrad=("wgrad_128_lean",)),
    _c("C2-342x14x14-128-256", (342, 14, 14, 128, 256, 3, 1, 1), fwd=("wide",), dgrad=("big_t",),
       wgrad=("wgrad_128",)),
    _c("C3-256x8x32-128-256-nonsquare", (256, 8, 32, 128, 256, 3, 1, 1), fwd=("wide",), dgrad=("big_t",),
       wgrad=("wgrad_big_lean",)),
    # D: conv_dgrad_s2_kernel (all four parity classes per workgroup)
    _c("D1-2x16x16-64-128-s2", (2, 16, 16, 64, 128, 3, 2, 1), fwd=("gemm_64x128",), dgrad=("dgrad_s2",),
       wgrad=("wgrad_128_lean",), even=True),
    _c("D2-6x14x14-64-128-s2", (6, 14, 14, 64, 128, 3, 2, 1), fwd=("gemm_64x128",), dgrad=("dgrad_s2",),
       wgrad=("wgrad_128",), even=True),
    _c("D3-3x8x16-128-256-s2-nonsquare", (3, 8, 16, 128, 256, 3, 2, 1), fwd=("gemm_64x128",),
       dgrad=("dgrad_s2",), wgrad=("wgrad_big",), even=True),
    _c("D4-1024x16x16-128-256-s2", (1024, 16, 16, 128, 256, 3, 2, 1), fwd=("wide",), dgrad=("dgrad_s2",),
       wgrad=("wgrad_big_lean",), even=True),
    # E: stride-2 data gradients by parity-class launches
    _c("E1-3x7x7-64-64-s2-odd", (3, 7, 7, 64, 64, 3, 2, 1), fwd=("gemm_64x64",), dgrad=("gemm_t_64x64",),
       wgrad=("wgrad_64",), even=True),
    _c("E2-D1-merged", (2, 16, 16, 64, 128, 3, 2, 1), s2=False, fwd=("gemm_64x128",), dgrad=("gemm_t_64x64",),
       wgrad=("wgrad_128_lean",), even=True),
    _c("E3-D2-merged", (6, 14, 14, 64, 128, 3, 2, 1), s2=False, fwd=("gemm_64x128",), dgrad=("gemm_t_64x64",),
       wgrad=("wgrad_128",), even=True),
    _c("E4-D3-merged", (3, 8, 16, 128, 256, 3, 2, 1), s2=False, fwd=("gemm_64x128",), dgrad=("gemm_t_64x128",),
       wgrad=("wgrad_big",), even=True),
    # phase mode in the large tiles: 4 x 64 tiles -> big, 4 x 256 tiles -> wide
    _c("E5-256x16x16-128-256-phase-big", (256, 16, 16, 128, 256, 3, 2, 1), s2=False, fwd=("gemm_64x128",),
       dgrad=("big_t",), wgrad=("wgrad_big_lean",), even=True),
    _c("E6-D4-phase-wide", (1024, 16, 16, 128, 256, 3, 2, 1), s2=False, fwd=("wide",), dgrad=("wide_t",),
       wgrad=("wgrad_big_lean",), even=True),
    _c("E7-2x16x16-64-128-1x1s2", (2, 16, 16, 64, 128, 1, 2, 0), fwd=("gemm_64x128",), dgrad=("gemm_t_64x64",),
       wgrad=("wgrad_128_lean",), even=True),
    _c("E8-64x16x16-128-256-1x1s2", (64, 16, 16, 128, 256, 1, 2, 0), fwd=("gemm_64x128",),
       dgrad=("gemm_t_64x128",), wgrad=("wgrad_big_lean",), even=True),
    # F: weight gradient
    _c("F1-64x16x16-128-256", (64, 16, 16, 128, 256, 3, 1, 1), fwd=("gemm_64x128",), dgrad=("gemm_t_64x128",),
       wgrad=("wgrad_big_lean",)),
    # M = 12,800 = 200 stages of 64 rows
    _c("F2-50x16x16-128-256", (50, 16, 16, 128, 256, 3, 1, 1), fwd=("gemm_64x128",), dgrad=("gemm_t_64x128",),
       wgrad=("wgrad_big_lean",)),
    _c("F3-6x14x14-128-256", (6, 14, 14, 128, 256, 3, 1, 1), fwd=("gemm_64x128",), dgrad=("gemm_t_64x128",),
       wgrad=("wgrad_128",)),
    _c("F4-64x4x4-512-512", (64, 4, 4, 512, 512, 3, 1, 1), fwd=("gemm_64x128",), dgrad=("gemm_t_64x128",),
       wgrad=("wgrad_big_lean",)),
    _c("F5-64x8x8-256-512-s2", (64, 8, 8, 256, 512, 3, 2, 1), fwd=("gemm_64x128",), dgrad=("dgrad_s2",),
       wgrad=("wgrad_big_lean",)),
    _c("F6-5x6x6-64-128", (5, 6, 6, 64, 128, 3, 1, 1), fwd=("gemm_64x128",), dgrad=("gemm_t_64x64",),
       wgrad=("wgrad_128",)),
    # G: direct 3x3 kernels (W = 32, H % 8 == 0); each with its implicit-GEMM twin (direct path off)
    _c("G1-1x8x32-64", (1, 8, 32, 64, 64, 3, 1, 1), yf=False, fwd=("halo_fwd_c64",), dgrad=("halo_dgrad",),
       wgrad=("halo_wgrad",)),
    _c("G2-3x24x32-64", (3, 24, 32, 64, 64, 3, 1, 1), yf=False, fwd=("halo_fwd_c64",), dgrad=("halo_dgrad",),
       wgrad=("halo_wgrad",)),
    _c("G3-5x8x32-8", (5, 8, 32, 8, 64, 3, 1, 1), yf=False, fwd=("halo_fwd_c8",), dgrad=("gemm_t_64x64",),
       wgrad=("wgrad_64_lean",)),
    # 260 tiles on 256 CUs: four workgroups take two tiles, the others one
    _c("G4-65x32x32-64", (65, 32, 32, 64, 64, 3, 1, 1), yf=False, fwd=("halo_fwd_c64",), dgrad=("halo_dgrad",),
       wgrad=("halo_wgrad",)),
    _c("G5-65x32x32-8", (65, 32, 32, 8, 64, 3, 1, 1), yf=False, fwd=("halo_fwd_c8",), dgrad=("gemm_t_128x64",),
       wgrad=("wgrad_64_lean",)),
]
CASES_BY_NAME = {c.name: c for c in CASES}
assert len(CASES_BY_NAME) == len(CASES)

# The ResNet engine's FC layer over more than 16 classes (kept apart from CASES, which other tables
# index): 37 rows of 512 features, a bias, and both gradients reading dy at the engine's dlogits
# stride (ops.cnn.logit_ld: 128 for 100 classes, 256 for 250).  The first shapes with a partial
# column tile after a full one (100 = 64 + 36, 250 = 128 + 122) and with an FC data gradient wider
# than 16 channels.
FC_CASES = (
    _c("H1-fc-37x512-100", (37, 1, 1, 512, 100, 1, 1, 0), fwd=("gemm_64x128",), dgrad=("gemm_t_64x128",),
       wgrad=("wgrad_128",), bias=True, ldd=128),
    _c("H2-fc-37x512-250", (37, 1, 1, 512, 250, 1, 1, 0), fwd=("gemm_64x128",), dgrad=("gemm_t_64x128",),
       wgrad=("wgrad_128",), bias=True, ldd=256),
)


def gemm_twin(case: Case) -> Case:
    """The same G case through the implicit GEMM (direct path off); families not asserted by name
    beyond 'no direct kernel', which :func:`run_case` checks for every halo=False case."""
    return dataclasses.replace(case, name=case.name + "-gemm", halo=False, fwd=(), dgrad=(), wgrad=())


# named subsets run by scripts/conv_exact_check.py in a fresh process
SUBSETS = {
    # deterministic build: one case each of B, C, D, F, G (fixed-point sums exact on integers)
    "det": ["B2-342x14x14-128-128", "C2-342x14x14-128-256", "D2-6x14x14-64-128-s2", "F2-50x16x16-128-256",
            "G4-65x32x32-64"],
    # SL_GEMM_SMALLM=1: the 128-row conv_gemm_kernel instantiations at small M with row tails
    "smallm": [c.name for c in CASES if c.smallm],
}


# ---------------------------------------------------------------------------------------------
# operands and reference
# ---------------------------------------------------------------------------------------------
def _ints(shape, lo, hi, density, gen, device):
    v = torch.randint(lo, hi + 1, shape, generator=gen, device=device, dtype=torch.int32)
    keep = torch.rand(shape, generator=gen, device=device) < density
    return (v * keep).to(torch.bfloat16)


def operands(case: Case, device="cpu", seed: int = 0) -> dict:
    """Integer-valued bf16 operands of a case: x [N,H,W,C], w [cout,k,k,C], dy [N,OH,OW,cout],
    add [N,H,W,C]; dw0 fp32 [cout,k,k,C] (the non-zero integers the weight gradient accumulates
    onto); for ``even`` cases a shortcut's dys [N,OH,OW,cout] and 1x1 weights wsc [cout,C]."""
    n, h, w, c, cout, k, s, p = case.shape
    oh, ow = case.out_hw()
    d = case.density()
    gen = torch.Generator(device=device).manual_seed(1000 + seed)
    o = {
        "x": _ints((n, h, w, c), -2, 2, d, gen, device),
        "w": _ints((cout, k, k, c), -1, 1, d, gen, device),
        "dy": _ints((n, oh, ow, cout), -2, 2, d, gen, device),
        "add": _ints((n, h, w, c), -2, 2, 1.0, gen, device),
        "dw0": torch.randint(-3, 4, (cout, k, k, c), generator=gen, device=device).float(),
    }
    if case.even:
        o["dys"] = _ints((n, oh, ow, cout), -2, 2, d, gen, device)
        o["wsc"] = _ints((cout, c), -1, 1, d, gen, device)
    return o


def reference(x, w, dy, stride: int, pad: int, chunk_bytes: int = 64 << 20):
    """float64 y [N,OH,OW,cout], dx [N,H,W,C], dw [cout,k,k,C] of the convolution, from the
    definition: per tap a shifted, strided slice of the zero-padded input and one float64 matmul
    (no convolution library, no autograd), in chunks over N."""
    n, h, wd, c = x.shape
    cout, kh_, kw_, _ = w.shape
    oh, ow = (h + 2 * pad - kh_) // stride + 1, (wd + 2 * pad - kw_) // stride + 1
    dev = x.device
    w64 = w.to(torch.float64)
    y = torch.empty(n, oh, ow, cout, dtype=torch.float64, device=dev)
    dx = torch.empty(n, h, wd, c, dtype=torch.float64, device=dev)
    dw = torch.zeros(cout, kh_, kw_, c, dtype=torch.float64, device=dev)
    per_img = 8 * max((h + 2 * pad) * (wd + 2 * pad) * c, oh * ow * max(c, cout))
    step = max(1, min(n, chunk_bytes // per_img))
    for n0 in range(0, n, step):
        n1 = min(n, n0 + step)
        xp = F.pad(x[n0:n1].to(torch.float64), (0, 0, pad, pad, pad, pad))  # zero padding of H and W
        dyc = dy[n0:n1].to(torch.float64).reshape(-1, cout)
        yc = torch.zeros((n1 - n0) * oh * ow, cout, dtype=torch.float64, device=dev)
        dxp = torch.zeros_like(xp)
        for kh in range(kh_):
            for kw in range(kw_):
                hs = slice(kh, kh + (oh - 1) * stride + 1, stride)
                ws = slice(kw, kw + (ow - 1) * stride + 1, stride)
                sl = xp[:, hs, ws, :].reshape(-1, c)          # x[n, oh s + kh - pad, ow s + kw - pad, :]
                wt = w64[:, kh, kw, :]                        # [cout, C]
                yc += sl @ wt.t()
                dw[:, kh, kw, :] += dyc.t() @ sl
                dxp[:, hs, ws, :] += (dyc @ wt).view(n1 - n0, oh, ow, c)
        y[n0:n1] = yc.view(n1 - n0, oh, ow, cout)
        dx[n0:n1] = dxp[:, pad:pad + h, pad:pad + wd, :]
    return y, dx, dw


def case_reference(case: Case, o: dict) -> dict:
    """Every expected output of a case, float64, on the operands' device."""
    n, h, w, c, cout, k, s, p = case.shape
    y, dx, dw = reference(o["x"], o["w"], o["dy"], s, p)
    y2 = y.reshape(-1, cout)
    r = {"y": y, "dx": dx, "dx_add": dx + o["add"].double(), "dw": dw + o["dw0"].double(),
         "stats": torch.cat([y2.sum(0), (y2 * y2).sum(0)])}
    if case.even:
        # 1x1 / stride-2 / pad-0 shortcut: its data gradient lives at the (even, even) positions
        ev = o["dys"].double() @ o["wsc"].double()  # [N,OH,OW,C]
        r["even"] = ev
        if k == 3:
            full = dx.clone()
            full[:, ::2, ::2] += ev
            r["dx_even"] = full
    return r


def check_bounds(case: Case, ref: dict) -> dict:
    """The conditions that make the comparison exact, asserted on the reference: every bf16
    output at most 256 in magnitude (before and after the add), every fp32 output below 2^24.
    Returns the maxima."""
    m = {"y": float(ref["y"].abs().max()), "dx": float(ref["dx"].abs().max()),
         "dx_add": float(ref["dx_add"].abs().max()), "stats": float(ref["stats"].abs().max()),
         "dw": float(ref["dw"].abs().max())}
    if "even" in ref:
        m["even"] = float(ref["even"].abs().max())
    if "dx_even" in ref:
        m["dx_even"] = float(ref["dx_even"].abs().max())
    for key in ("y", "dx", "dx_add", "even", "dx_even"):
        assert m.get(key, 0.0) <= BF16_EXACT, (case.name, key, m)
    for key in ("stats", "dw"):
        assert m[key] < F32_EXACT, (case.name, key, m)
    assert m["y"] > 0 and m["dw"] > 0 and (m["dx"] > 0 or not case.do_dgrad), (case.name, m)  # not vacuous
    return m


# ---------------------------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------------------------
@dataclass
class Mismatch:
    what: str
    count: int
    total: int
    index: tuple               # (n, oh, ow, channel) for pixel tensors, the plain index otherwise
    got: float
    want: float
    row: int = -1              # GEMM row of that pixel
    tiles: dict = field(default_factory=dict)   # tile height -> (tile, row within the tile)
    cls: tuple = ()            # parity class (ph, pw) of a stride-2 data gradient's pixel
    cls_row: int = -1          # GEMM row within that class
    cls_tiles: dict = field(default_factory=dict)

    def __str__(self):
        s = "%s: %d of %d elements differ; first at %s: got %r, want %r" % (
            self.what, self.count, self.total, self.index, self.got, self.want)
        if self.row >= 0:
            s += "; GEMM row %d = " % self.row + ", ".join(
                "%d-row tile %d row %d" % (t, a, b) for t, (a, b) in self.tiles.items())
            s += " (fragment row %d)" % (self.row % 16)
        if self.cls:
            s += "; parity class %s row %d = " % (self.cls, self.cls_row) + ", ".join(
                "%d-row tile %d row %d" % (t, a, b) for t, (a, b) in self.cls_tiles.items())
        return s


def _tiles(row):
    return {t: (row // t, row % t) for t in (256, 128, 64)}


def compare(got, ref, what: str = "", pixels: bool = True, parity: bool = False):
    """None when ``got`` equals the float64 ``ref`` element for element (``torch.equal``, no
    tolerance; a NaN never equals), else a :class:`Mismatch` locating the first differing
    element.  pixels: the tensors are [N,OH,OW,channels] (or [N*OH*OW, channels] with ref giving
    the shape); parity: a stride-2 data gradient, whose pixel (oh, ow) belongs to class
    (oh & 1, ow & 1) with its own row numbering."""
    g = got.detach().to(torch.float64).reshape(ref.shape)
    if torch.equal(g, ref):
        return None
    bad = (g != ref) | torch.isnan(g)
    flat = int(torch.nonzero(bad.reshape(-1))[0])
    idx, rem = [], flat
    for dim in reversed(ref.shape):
        idx.append(rem % dim)
        rem //= dim
    idx = tuple(reversed(idx))
    m = Mismatch(what, int(bad.sum()), ref.numel(), idx, float(g.reshape(-1)[flat]), float(ref.reshape(-1)[flat]))
    if pixels and ref.dim() == 4:
        n, oh, ow, _ = idx
        _, hh, ww, _ = ref.shape
        m.row = (n * hh + oh) * ww + ow
        m.tiles = _tiles(m.row)
        if parity:
            ph, pw = oh & 1, ow & 1
            hp, wp = (hh - ph + 1) // 2, (ww - pw + 1) // 2
            m.cls = (ph, pw)
            m.cls_row = (n * hp + oh // 2) * wp + ow // 2
            m.cls_tiles = _tiles(m.cls_row)
    return m


# ---------------------------------------------------------------------------------------------
# driver (GPU)
# ---------------------------------------------------------------------------------------------
def _next_pow2(v: int) -> int:
    return 1 << (v - 1).bit_length()


def run_case(case: Case, device="cuda", smallm: bool = False, keep: bool = False) -> dict:
    """Run one case through the launchers and compare every output with the reference.
    Returns {"failures": [str], "seen": {op: [families]}, "maxima": {...}, "density": d} and,
    with ``keep``, the raw outputs under "out".  ``smallm``: the process runs with
    SL_GEMM_SMALLM=1, so the case's ``smallm`` families are the expected ones."""
    from ..ops import _native, cnn as K

    n, h, w, c, cout, k, s, p = case.shape
    oh, ow = case.out_hw()
    o = operands(case, device)
    ref = case_reference(case, o)
    maxima = check_bounds(case, ref)
    det = K.deterministic()
    fails, seen, out = [], {}, {}
    want_fwd, want_dgrad = (case.smallm if smallm else (case.fwd, case.dgrad))

    def check(m):
        if m is not None:
            fails.append(str(m))

    def families(op, want):
        got = K.conv_kernels_seen(clear=True)
        seen[op] = sorted(got)
        missing = set(want) - got
        if missing:
            fails.append("%s: expected kernel family %s, launched %s" % (op, sorted(missing), sorted(got)))
        if not case.halo and any(f.startswith("halo") for f in got):
            fails.append("%s: direct kernel %s ran with the direct path off" % (op, sorted(got)))

    def nan_like(*shape, dtype=torch.bfloat16):
        return torch.full(shape, float("nan"), dtype=dtype, device=device)  # every element must be written

    _native.call("sl_conv_set_halo", 1 if case.halo else 0)
    _native.call("sl_conv_set_s2", 1 if case.s2 else 0)
    try:
        # forward: y bf16, yf fp32, per-channel sum and sum of squares
        ldy = (cout + 7) // 8 * 8
        y = nan_like(n, oh, ow, ldy)
        yf = nan_like(n * oh * ow, cout, dtype=torch.float32) if case.yf else None
        sbuf = torch.zeros(K.rsum_floats(2 * cout), device=device)
        K.conv_kernels_seen(clear=True)
        K.conv_fwd(o["x"], o["w"], cout, k, s, p, y=y, yf=yf, stats=sbuf)
        torch.cuda.synchronize()
        families("fwd", want_fwd)
        check(compare(y[..., :cout], ref["y"], "y (bf16)"))
        if yf is not None:
            check(compare(yf, ref["y"], "yf (fp32)"))
        check(compare(K.rsum_result(sbuf, 2 * cout), ref["stats"], "stats (sum | sum of squares per channel)",
                      pixels=False))
        out["y"] = y[..., :cout]
        if case.bias:  # the FC form: a second forward with an integer bias, fp32 and bf16 outputs
            gen = torch.Generator(device=device).manual_seed(7)
            bias = torch.randint(-3, 4, (cout,), generator=gen, device=device).float()
            yb_ref = ref["y"] + bias.double()
            assert float(yb_ref.abs().max()) <= BF16_EXACT, case.name
            yb, yfb = nan_like(n, oh, ow, ldy), nan_like(n * oh * ow, cout, dtype=torch.float32)
            K.conv_fwd(o["x"], o["w"], cout, k, s, p, y=yb, yf=yfb, bias=bias)
            torch.cuda.synchronize()
            check(compare(yb[..., :cout], yb_ref, "y + bias (bf16)"))
            check(compare(yfb, yb_ref, "yf + bias (fp32)"))

        # the gradient dy padded to the launchers' channel strides: a multiple of 8 for the weight
        # gradient; a power of two for the data gradient (fill_geom needs one for its source)
        ldw = case.ldd or ldy
        dyp = torch.zeros(n, oh, ow, ldw, dtype=torch.bfloat16, device=device)
        dyp[..., :cout] = o["dy"]
        ldd = case.ldd or _next_pow2(ldy)
        assert ldd >= cout and ldd & (ldd - 1) == 0 and ldw % 8 == 0, (case.name, ldd, ldw)

        def padded(t, ld):  # [.., cout] -> [.., ld]
            if ld == t.shape[-1]:
                return t.contiguous()
            z = torch.zeros(*t.shape[:-1], ld, dtype=t.dtype, device=device)
            z[..., :t.shape[-1]] = t
            return z

        if case.do_dgrad:
            dyd = padded(o["dy"], ldd)
            wt = padded(o["w"].reshape(cout, k * k, c).permute(2, 1, 0), ldd).reshape(-1)  # [C][tap][ldd]
            par = s == 2
            dx = nan_like(n, h, w, c)
            K.conv_kernels_seen(clear=True)
            K.conv_dgrad(dyd, wt, c, k, s, p, dx, add=o["add"])
            torch.cuda.synchronize()
            families("dgrad", want_dgrad)
            check(compare(dx, ref["dx_add"], "dx + add", parity=par))
            out["dx_add"] = dx
            dx0 = nan_like(n, h, w, c)
            K.conv_dgrad(dyd, wt, c, k, s, p, dx0)
            torch.cuda.synchronize()
            check(compare(dx0, ref["dx"], "dx", parity=par))
            if case.even:
                # the shortcut's gradient at the even positions only, the rest left untouched ...
                wst = padded(o["wsc"].t(), ldd).reshape(-1) if k == 3 else wt   # [C][1][ldd]
                dys = padded(o["dys"], ldd) if k == 3 else dyd
                ev_ref = ref["even"] if k == 3 else ref["dx"][:, ::2, ::2]
                got = nan_like(n, h, w, c)
                K.conv_kernels_seen(clear=True)
                K.conv_dgrad_s2_even(dys, wst, c, got)
                torch.cuda.synchronize()
                seen["even"] = sorted(K.conv_kernels_seen(clear=True))
                check(compare(got[:, ::2, ::2], ev_ref, "even-position shortcut gradient"))
                rest = got.clone()
                rest[:, ::2, ::2] = float("nan")
                if not bool(torch.isnan(rest.float()).all()):
                    fails.append("conv_dgrad_s2_even wrote outside the (even, even) positions")
                if k == 3:  # ... then the 3x3 gradient writes every position and adds at the even ones
                    K.conv_dgrad(dyd, wt, c, k, s, p, got, add=got, add_even=True)
                    torch.cuda.synchronize()
                    families("dgrad_add_even", want_dgrad)
                    check(compare(got, ref["dx_even"], "dx + add_even", parity=True))

        # weight gradient onto a non-zero dw: atomics (not in the deterministic build, which has
        # none) and the slab + ordered reduce, for each split-K target
        want_w = set(case.wgrad)
        for tw in case.target_wgs:
            K.conv_kernels_seen(clear=True)
            if not det:
                dw = o["dw0"].clone()
                K.conv_wgrad(o["x"], dyp, cout, k, s, p, dw, target_wgs=tw)
                torch.cuda.synchronize()
                check(compare(dw, ref["dw"], "dw (atomics, target_wgs=%d)" % tw, pixels=False))
            ws = K.WgradWorkspace(device)
            K.conv_wgrad(o["x"], dyp, cout, k, s, p, o["dw0"].clone(), target_wgs=tw, ws=ws)  # sizes the slab
            ws.grow()
            dw2 = o["dw0"].clone()
            K.conv_wgrad(o["x"], dyp, cout, k, s, p, dw2, target_wgs=tw, ws=ws)
            torch.cuda.synchronize()
            families("wgrad[%d]" % tw, want_w)
            check(compare(dw2, ref["dw"], "dw (slab, target_wgs=%d)" % tw, pixels=False))
            out["dw"] = dw2
    finally:
        _native.call("sl_conv_set_halo", 1)
        _native.call("sl_conv_set_s2", 1)
    r = {"name": case.name, "failures": fails, "seen": seen, "maxima": maxima, "density": case.density(),
         "deterministic_build": bool(det)}
    if keep:
        r["out"] = out
    return r
