"""SE-ResNeXt-50 32x4d on the MI355X.

Part A -- the five squeeze-and-excitation entry points alone (mh_se_gate_fwd / mh_se_apply_fwd / mh_se_apply_bwd_reduce / mh_se_gate_bwd /
  mh_se_apply_bwd; the squeeze itself is mh_avgpool_fwd) against their float64 statement on the CPU: bit for bit on operands whose
  products and sums are representable, inside derived bounds on random operands (the derivation: _gate_reference's docstring), a
  saturated gate, the same bits on every call, and refusals that write nothing.
Part B -- ``SEResNeXt50_32x4d(layers=(1, 1, 1, 1))`` forward + backward against the float64 composition of tests/test_resnext_gpu.py part B
  (restated here) extended by the SE block: the same 16-bit storage points (straight-through) plus u = q(bn3(.)) and
  out = q(relu(u * s + shortcut)), the gate in f32; the same bars and the same seed rule.  Then gradient accumulation, the classifier under
  the fused Adam, Kevin's three-tower model, ``SEResNeXt50_32x4d_BH``, and the launch lists of the ResNeXt and the SE-ResNeXt step."""
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from conftest import parity_log

pytestmark = pytest.mark.gpu
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("T16", [F16, BF16], ids=["fp16", "bf16"])
HALF_ULP = {F16: 2.0 ** -11, BF16: 2.0 ** -8}          # half an ulp of the one output rounding, relative
HALF_SUBNORMAL = {F16: 2.0 ** -25, BF16: 2.0 ** -134}   # ... and absolute below the smallest normal (2^-14 / 2^-126), where the spacing is fixed
U32 = 2.0 ** -24                                        # f32's unit roundoff
MH_EINVAL, MH_ESHAPE = 1, 2
SE_ENTRY_POINTS = ("mh_se_gate_fwd", "mh_se_apply_fwd", "mh_se_apply_bwd_reduce", "mh_se_gate_bwd", "mh_se_apply_bwd")

# (B, HW, C, R)
CASES = {
    "pixel": (1, 1, 64, 8),                # a single pixel: the mean is the value
    "odd_hw": (2, 35, 64, 4),              # odd HW
    "c200_r13": (3, 9, 200, 13),           # C not a multiple of 64 (the last 64-column group has one 8-channel chunk); odd R
    "layer4": (2, 49, 2048, 128),          # layer4's real HW, C and R
    "layer1": (2, 3136, 256, 16),          # layer1's real HW: the longest column sum -- seven trips of the 16-wave reduce, 25 rows a thread
    # beyond the issue's list: the sizes at which the code takes another path.  The reduce's 4-wave form with more than one trip (it is
    # chosen from B * ceil(C / 64) >= 512, as layer3 of the real tower at batch 32), at the largest C (the fc1 gradient's 16-column form);
    "wide_c4096": (8, 137, 4096, 8),
    # the fc1 gradient's 2- and 4-column forms (256 < C <= 512, 512 < C <= 1024), C = 1000 no multiple of 64
    "c512": (2, 5, 512, 32),
    "c1000": (2, 3, 1000, 64),
}
CASE = pytest.mark.parametrize("case", list(CASES))


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import multimodal_propaganda_meme_classification_amd as m
    return m


def _lib(pkg, T16):
    return pkg._lib.load("fp16" if T16 == F16 else "bf16")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _name(T16):
    return "fp16" if T16 == F16 else "bf16"


def _bits(t):
    return t.contiguous().view(torch.int16)


GUARD16, GUARD32, PAD = 7.0, 12345.0, 64


class _Dev:
    """the device side of part A: every output has PAD guard words behind it, checked after each launch"""

    def __init__(self, pkg, T16, B, HW, C, R):
        self.pkg, self.lib, self.T16, self.B, self.HW, self.C, self.R = pkg, _lib(pkg, T16), T16, B, HW, C, R

    def _out16(self):
        return torch.full((self.B * self.HW * self.C + PAD,), GUARD16, dtype=self.T16, device="cuda")

    def _out32(self, n):
        return torch.full((n + PAD,), GUARD32, dtype=F32, device="cuda")

    def _take(self, what, buf, n, shape):
        guard = GUARD16 if buf.dtype == self.T16 else GUARD32
        assert bool((buf[n:] == guard).all()), f"{what} wrote past its output"
        return buf[:n].view(shape).cpu()

    def act(self, t):          # [B, HW, C] float64 -> 16-bit device matrix
        return t.reshape(self.B * self.HW, self.C).to(self.T16).cuda()

    def gate_fwd(self, pooled, w1, b1, w2, b2):
        B, C, R = self.B, self.C, self.R
        d = [t.to(F32).contiguous().cuda() for t in (pooled, w1, b1, w2, b2)]
        hidden, s = self._out32(B * R), self._out32(B * C)
        self.pkg._lib.check(self.lib.mh_se_gate_fwd(*[t.data_ptr() for t in d], hidden.data_ptr(), s.data_ptr(), B, C, R, _st()), "mh_se_gate_fwd")
        torch.cuda.synchronize()
        return self._take("mh_se_gate_fwd", hidden, B * R, (B, R)), self._take("mh_se_gate_fwd", s, B * C, (B, C))

    def apply_fwd(self, u, s, sc):
        B, HW, C = self.B, self.HW, self.C
        ud, sd, scd, y = self.act(u), s.to(F32).contiguous().cuda(), self.act(sc), self._out16()
        self.pkg._lib.check(self.lib.mh_se_apply_fwd(ud.data_ptr(), sd.data_ptr(), scd.data_ptr(), y.data_ptr(), B, HW, C, _st()), "mh_se_apply_fwd")
        torch.cuda.synchronize()
        return self._take("mh_se_apply_fwd", y, B * HW * C, (B, HW, C))

    def bwd_reduce(self, dy, y, u):
        B, HW, C = self.B, self.HW, self.C
        dyd, yd, ud, g, ds = self.act(dy), self.act(y), self.act(u), self._out16(), self._out32(B * C)
        self.pkg._lib.check(self.lib.mh_se_apply_bwd_reduce(dyd.data_ptr(), yd.data_ptr(), ud.data_ptr(), g.data_ptr(), ds.data_ptr(), B, HW, C, _st()),
                            "mh_se_apply_bwd_reduce")
        torch.cuda.synchronize()
        return self._take("mh_se_apply_bwd_reduce", g, B * HW * C, (B, HW, C)), self._take("mh_se_apply_bwd_reduce", ds, B * C, (B, C))

    def gate_bwd(self, ds, s, hidden, pooled, w1, w2, alpha=1.0, accumulate=0, targets=None):
        """-> dpooled, dw1, db1, dw2, db2; `targets`: four f32 CPU tensors the parameter gradients start from"""
        B, C, R = self.B, self.C, self.R
        d = [t.to(F32).contiguous().cuda() for t in (ds, s, hidden, pooled, w1, w2)]
        sizes = (R * C, R, C * R, C)
        outs = [self._out32(n) for n in sizes]
        if targets is not None:
            for o, t, n in zip(outs, targets, sizes):
                o[:n] = t.reshape(-1).cuda()
        dp = self._out32(B * C)
        self.pkg._lib.check(self.lib.mh_se_gate_bwd(*[t.data_ptr() for t in d], dp.data_ptr(), *[o.data_ptr() for o in outs], B, C, R, alpha,
                                                    accumulate, _st()), "mh_se_gate_bwd")
        torch.cuda.synchronize()
        shapes = ((R, C), (R,), (C, R), (C,))
        return (self._take("mh_se_gate_bwd", dp, B * C, (B, C)),) + tuple(self._take("mh_se_gate_bwd", o, n, sh) for o, n, sh in zip(outs, sizes, shapes))

    def apply_bwd(self, g, s, dpooled):
        B, HW, C = self.B, self.HW, self.C
        gd, sd, dpd, du = self.act(g), s.to(F32).contiguous().cuda(), dpooled.to(F32).contiguous().cuda(), self._out16()
        self.pkg._lib.check(self.lib.mh_se_apply_bwd(gd.data_ptr(), sd.data_ptr(), dpd.data_ptr(), du.data_ptr(), B, HW, C, _st()), "mh_se_apply_bwd")
        torch.cuda.synchronize()
        return self._take("mh_se_apply_bwd", du, B * HW * C, (B, HW, C))


# ---------------------------------------------------------------------------------------------------------------------
# A. the kernels alone
# ---------------------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _exact_operands(case):
    """u, dy in [-3, 3], shortcut in [-4, 4] (integers), s in {0.5, 1, 2}, dpooled = HW * k with k in [-2, 2]: u * s + shortcut is a multiple
    of 0.5 of size <= 10 (5 significant bits), g * s + dpooled / HW one of size <= 8, g * u an integer of size <= 9 whose HW <= 3136 term sum
    stays below 28 224 < 2^24 -- every value is representable in bf16, fp16 and f32, so every order of evaluation gives the float64 result."""
    B, HW, C, _ = CASES[case]
    gen = torch.Generator().manual_seed(100 + list(CASES).index(case))
    ri = lambda shape, a: torch.randint(-a, a + 1, shape, generator=gen).to(F64)
    u, sc, dy = ri((B, HW, C), 3), ri((B, HW, C), 4), ri((B, HW, C), 3)
    s = torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, (B, C), generator=gen)]
    dpooled = ri((B, C), 2) * HW
    y = F.relu(u * s[:, None] + sc)
    g = torch.where(y > 0, dy, torch.zeros_like(dy))
    ds = (g * u).sum(1)
    du = g * s[:, None] + (dpooled / HW)[:, None]
    assert float(ds.abs().max()) < 2 ** 24 and float(y.max()) <= 10 and float(du.abs().max()) <= 8
    return dict(u=u, sc=sc, dy=dy, s=s, dpooled=dpooled, y=y, g=g, ds=ds, du=du)


@DTYPES
@CASE
def test_se_apply_kernels_are_exact_on_representable_operands(pkg, case, T16):
    """mh_se_apply_fwd, g, ds and mh_se_apply_bwd equal the float64 statement bit for bit; y == 0 masks (strict > 0), with a nonzero dy at such
    an element in every case; the guard words behind every output stay unwritten (_Dev._take)."""
    o = _exact_operands(case)
    B, HW, C, R = CASES[case]
    d = _Dev(pkg, T16, B, HW, C, R)
    y = d.apply_fwd(o["u"], o["s"], o["sc"])
    want = o["y"].to(T16)
    assert torch.equal(_bits(y), _bits(want)), f"apply_fwd: {int((y != want).sum())} of {y.numel()} elements differ"
    at_zero = (o["y"] == 0) & (o["dy"] != 0)
    assert bool(at_zero.any()) and bool((o["u"] * o["s"][:, None] + o["sc"] == 0)[at_zero].any()), "no y == 0 element tests the strict mask"
    g, ds = d.bwd_reduce(o["dy"], o["y"], o["u"])
    assert torch.equal(_bits(g), _bits(o["g"].to(T16))), f"g: {int((g != o['g'].to(T16)).sum())} of {g.numel()} elements differ"
    assert bool((g[at_zero] == 0).all())
    assert torch.equal(ds.to(F64), o["ds"]), f"ds: {int((ds.to(F64) != o['ds']).sum())} of {ds.numel()} sums differ"
    du = d.apply_bwd(o["g"], o["s"], o["dpooled"])
    assert torch.equal(_bits(du), _bits(o["du"].to(T16))), f"apply_bwd: {int((du != o['du'].to(T16)).sum())} of {du.numel()} elements differ"


@DTYPES
def test_se_reduce_copies_the_bits_of_dy(pkg, T16):
    """g is dy's bit pattern where y > 0 (a negative zero and the smallest subnormal included), +0 elsewhere -- also where y is -0 or negative"""
    B, HW, C = 1, 3, 8
    dy = torch.tensor([-0.0, 1.0, -2.0, 3.0, 0.5, -0.25, 4.0, 1.5], dtype=T16).repeat(B * HW, 1)
    dy[1, 0] = torch.tensor([1], dtype=torch.int16).view(T16)[0]          # the smallest subnormal
    y = torch.tensor([1.0, 0.0, -0.0, 2.0, -1.0, 1.0, 0.0, 3.0], dtype=T16).repeat(B * HW, 1)
    y[1, 0] = torch.tensor([1], dtype=torch.int16).view(T16)[0]
    u = torch.ones((B * HW, C), dtype=T16)
    d = _Dev(pkg, T16, B, HW, C, 8)
    g, ds = d.bwd_reduce(dy.to(F64).view(B, HW, C), y.to(F64).view(B, HW, C), u.to(F64).view(B, HW, C))
    want = torch.where(y > 0, dy, torch.zeros_like(dy))
    assert torch.equal(_bits(g.view(B * HW, C)), _bits(want))
    assert int(_bits(g.view(B * HW, C))[0, 0]) == int(_bits(dy)[0, 0]) != 0          # -0.0 kept its sign bit
    assert torch.equal(ds.view(C).to(F64), want.to(F64).sum(0))


def _gate_forward64(pooled, w1, b1, w2, b2):
    hidden = F.relu(pooled @ w1.t() + b1)
    return hidden, torch.sigmoid(hidden @ w2.t() + b2)


def _gate_reference(pooled, w1, b1, w2, b2, ds, arith=F64):
    """The gate in `arith` on the CPU with torch autograd over hidden = relu(w1 pooled + b1), s = sigmoid(w2 hidden + b2), and the bounds of
    an f32 evaluation of it.  Notation: u = 2^-24; |.| elementwise; an n-term f32 sum taken in any order (products fused or not) is within
    (n + 1) u sum|terms| of the exact one, its bias (or alpha) one term more.

    forward (mh_se_gate_fwd from pooled, w1, b1, w2, b2):
      E_h  = (C + 2) u (|w1| |pooled| + |b1|)                        hidden (the ReLU is 1-Lipschitz)
      E_a  = |w2| E_h + (R + 2) u (|w2| (hidden + E_h) + |b2|)       the pre-activation of the sigmoid
      E_s  = E_a / 4 + 4 u s                                         sigmoid' <= 1/4; expf is within 1 ulp = 2^-23 relative (the documented
             error of the accurate expf), which moves s = 1 / (1 + e) by e 2^-23 / (1 + e)^2 <= 2 u s; 1 + e and the division round once each
    backward (mh_se_gate_bwd from ds and the float64 hidden, s ROUNDED to f32 -- a relative u each; the test asserts hidden's mask survived):
      da   = ds s (1 - s);  E_da = u |ds| (s + 4 s (1 - s))          1 - s moves by u s; two products, the rounding of s, of 1 - s
      E_dh = E_da |w2| + (C + 2) u |da| |w2|                         dh = [hidden > 0] da w2
      dw2  : sum_b (E_da hidden + u |da| hidden) + (B + 2) u sum_b |da| hidden;      db2 : sum_b E_da + (B + 2) u sum_b |da|
      dw1  : sum_b E_dh |pooled| + (B + 2) u sum_b (|dh| + E_dh) |pooled|;           db1 : sum_b E_dh + (B + 2) u sum_b (|dh| + E_dh)
      dpooled : E_dh |w1| + (R + 2) u (|dh| + E_dh) |w1|             the same bound through the second layer
    Returns (values, bounds) as dicts; the values carry `arith`."""
    B, C = pooled.shape
    R = w1.shape[0]
    leaves = [t.to(arith).clone().requires_grad_(True) for t in (pooled, w1, b1, w2, b2)]
    p, a1, c1, a2, c2 = leaves
    hidden, s = _gate_forward64(p, a1, c1, a2, c2)
    val = dict(hidden=hidden.detach(), s=s.detach())
    if ds is not None:
        s.backward(ds.to(arith))
        val.update(dpooled=p.grad, dw1=a1.grad, db1=c1.grad, dw2=a2.grad, db2=c2.grad)
    if arith != F64:
        return val, None
    aw1, aw2, ap = w1.abs(), w2.abs(), pooled.abs()
    h, sv = val["hidden"], val["s"]
    E_h = (C + 2) * U32 * (ap @ aw1.t() + b1.abs())
    E_a = E_h @ aw2.t() + (R + 2) * U32 * ((h + E_h) @ aw2.t() + b2.abs())
    bound = dict(hidden=E_h, s=E_a / 4 + 4 * U32 * sv)
    if ds is not None:
        t = sv * (1 - sv)
        da = ds * t
        E_da = U32 * ds.abs() * (sv + 4 * t)
        mask = (h > 0).to(F64)
        dh = mask * (da @ w2)
        E_dh = mask * (E_da @ aw2 + (C + 2) * U32 * (da.abs() @ aw2))
        adh = dh.abs() + E_dh
        bound.update(dw2=(E_da + U32 * da.abs()).t() @ h + (B + 2) * U32 * (da.abs().t() @ h), db2=E_da.sum(0) + (B + 2) * U32 * da.abs().sum(0),
                     dw1=E_dh.t() @ ap + (B + 2) * U32 * (adh.t() @ ap), db1=E_dh.sum(0) + (B + 2) * U32 * adh.sum(0),
                     dpooled=E_dh @ aw1 + (R + 2) * U32 * (adh @ aw1))
    return val, bound


def _gate_backward32(ds, s, hidden, pooled, w1, w2):
    """mh_se_gate_bwd's statement evaluated in float32 on the CPU from the operands the device gets (alpha = 1): what the bounds of
    _gate_reference must hold for before the GPU is asked"""
    ds, s, hidden, pooled, w1, w2 = (t.to(F32) for t in (ds, s, hidden, pooled, w1, w2))
    da = ds * s * (1 - s)
    dh = (hidden > 0).to(F32) * (da @ w2)
    return dict(dpooled=dh @ w1, dw1=dh.t() @ pooled, db1=dh.sum(0), dw2=da.t() @ hidden, db2=da.sum(0))


@lru_cache(maxsize=None)
def _random_operands(case, T16):
    B, HW, C, R = CASES[case]
    gen = torch.Generator().manual_seed(700 + 2 * list(CASES).index(case) + (T16 == BF16))
    rn = lambda *shape: torch.randn(shape, generator=gen, dtype=F64)
    r16 = lambda *shape: rn(*shape).to(T16).to(F64)
    r32 = lambda t: t.to(F32).to(F64)
    u, sc, dy = r16(B, HW, C), r16(B, HW, C), r16(B, HW, C)
    pooled = r32(u.mean(1))
    w1, b1, w2, b2 = r32(rn(R, C) / C ** 0.5), r32(0.2 * rn(R)), r32(rn(C, R) / R ** 0.5), r32(0.2 * rn(C))
    ds = r32(rn(B, C) * HW ** 0.5)
    return dict(u=u, sc=sc, dy=dy, pooled=pooled, w1=w1, b1=b1, w2=w2, b2=b2, ds=ds)


def _rounding(ref, T16):
    """half an ulp of the 16-bit format at `ref`: 2^-p |ref|, and half the fixed spacing where the result is subnormal (fp16 below 6.1e-5:
    a masked element's du is dpooled / HW alone and lands there; 2^-p |ref| is not the format's precision at such a value)"""
    return (HALF_ULP[T16] * ref.abs()).clamp_min(HALF_SUBNORMAL[T16])


def _within(what, got, ref, bar, worst):
    got = got.to(F64)
    assert torch.isfinite(got).all(), what
    frac = float(((got - ref).abs() / bar.clamp_min(1e-300)).max())
    worst[what] = frac
    assert bool(((got - ref).abs() <= bar).all()), f"{what}: worst error {frac:.3g} x the bar"


@DTYPES
@CASE
def test_se_kernels_random_operands_within_derived_bounds(pkg, case, T16):
    """Random operands against float64 (torch autograd over the formulas): the 16-bit outputs y and du within 2^-p |ref| + 2 2^-24 sum|terms|
    (p = 11 fp16, 8 bf16: the one output rounding -- _rounding: half the subnormal spacing where the result is subnormal --, the fused
    multiply-add and, for du, the division); ds within HW 2^-24 sum_hw |g u|; hidden, s, dpooled and the four parameter gradients within
    _gate_reference's bounds.  Those bounds are asserted for the float32 CPU evaluation of the same statements first (the forward from its
    operands, the backward from the operands the device gets), before the GPU is touched: a bound the reference misses in float32 is no
    usable bound.  Measured on the MI355X (worst error / bar over the eight cases and both dtypes): see the parity log lines [se ...]."""
    o = _random_operands(case, T16)
    B, HW, C, R = CASES[case]
    gate = (o["pooled"], o["w1"], o["b1"], o["w2"], o["b2"])
    ref, bound = _gate_reference(*gate, o["ds"])
    h32, s32 = ref["hidden"].to(F32), ref["s"].to(F32)
    assert torch.equal(h32 > 0, ref["hidden"] > 0), "rounding hidden to f32 moved its mask: no usable input"
    cpu32, _ = _gate_reference(*gate, None, arith=F32)          # the forward in float32; the backward from the operands the device gets
    cpu32.update(_gate_backward32(o["ds"], s32, h32, o["pooled"], o["w1"], o["w2"]))
    for k, bar in bound.items():
        assert bool(((cpu32[k].to(F64) - ref[k]).abs() <= bar).all()), f"{k}: the float32 CPU evaluation misses the bound ({case})"
    d = _Dev(pkg, T16, B, HW, C, R)
    worst = {}
    hidden, s = d.gate_fwd(*gate)
    _within("hidden", hidden, ref["hidden"], bound["hidden"], worst)
    _within("s", s, ref["s"], bound["s"], worst)
    got = d.gate_bwd(o["ds"], s32, h32, o["pooled"], o["w1"], o["w2"])
    for k, t in zip(("dpooled", "dw1", "db1", "dw2", "db2"), got):
        _within(k, t, ref[k].view_as(t), bound[k].view_as(t), worst)
    # the three kernels over the activation, the gate taken from the float64 reference rounded to f32
    sv = s32.to(F64)[:, None]
    y_ref = F.relu(o["u"] * sv + o["sc"])
    y = d.apply_fwd(o["u"], s32, o["sc"])
    _within("y", y, y_ref, _rounding(y_ref, T16) + 2 * U32 * ((o["u"] * sv).abs() + o["sc"].abs()), worst)
    y16 = y_ref.to(T16).to(F64)
    g_ref = torch.where(y16 > 0, o["dy"], torch.zeros_like(o["dy"]))
    g, ds = d.bwd_reduce(o["dy"], y16, o["u"])
    assert torch.equal(_bits(g), _bits(g_ref.to(T16)))
    _within("ds", ds, (g_ref * o["u"]).sum(1), HW * U32 * (g_ref * o["u"]).abs().sum(1), worst)
    dp32 = ref["dpooled"].to(F32)
    du_ref = g_ref * sv + (dp32.to(F64) / HW)[:, None]
    du = d.apply_bwd(g_ref, s32, dp32)
    _within("du", du, du_ref, _rounding(du_ref, T16) + 2 * U32 * ((g_ref * sv).abs() + (dp32.to(F64) / HW).abs()[:, None]), worst)
    parity_log(f"[se {case} {_name(T16)}] worst error / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@DTYPES
def test_se_saturated_gate_is_finite_and_has_no_gradient_there(pkg, T16):
    """Pre-activations of +60 (columns 0, 1) and -60 (columns 2, 3; w2 = 0 there, b2 = +-60): s is finite -- exactly 1 on the + side,
    sigmoid(-60) = 8.8e-27 on the - side, as in float64 --, and the gate gradient of those columns is zero: exactly on the + side
    (1 - s = 0), below 1e-24 on the - side (|ds| s; float64 gives the same), while every other column keeps a gradient."""
    B, HW, C, R = 2, 1, 64, 8
    gen = torch.Generator().manual_seed(77)
    rn = lambda *shape: torch.randn(shape, generator=gen, dtype=F64).to(F32).to(F64)
    pooled, w1, b1, w2, b2, ds = rn(B, C), rn(R, C) / 8, 1.0 + rn(R).abs(), rn(C, R) / 3, 0.2 * rn(C), 1.0 + rn(B, C).abs()
    w2[:4] = 0.0
    b2[:2], b2[2:4] = 60.0, -60.0
    ref, bound = _gate_reference(pooled, w1, b1, w2, b2, ds)
    d = _Dev(pkg, T16, B, HW, C, R)
    hidden, s = d.gate_fwd(pooled, w1, b1, w2, b2)
    assert bool(torch.isfinite(s).all()) and bool((s[:, :2] == 1.0).all()) and bool((s[:, 2:4] > 0).all()) and bool((s[:, 2:4] < 1e-25).all())
    assert bool(((s.to(F64) - ref["s"]).abs() <= bound["s"]).all())
    dpooled, dw1, db1, dw2, db2 = d.gate_bwd(ds, s, hidden, pooled, w1, w2)
    for t in (dpooled, dw1, db1, dw2, db2):
        assert bool(torch.isfinite(t).all())
    assert bool((db2[:2] == 0).all()) and bool((dw2[:2] == 0).all())
    assert bool((db2[2:4].abs() < 1e-24).all()) and bool((dw2[2:4].abs() < 1e-24).all()) and bool((ref["db2"][2:4].abs() < 1e-24).all())
    assert bool((db2[4:].abs() > 1e-6).all()) and bool((dw2[4:].abs().sum(1) > 1e-6).all()), "a live column lost its gate gradient"
    # a gate saturated beyond expf's range: exactly 0 and 1, no NaN, no gradient
    b2[:2], b2[2:4] = 200.0, -200.0
    _, s = d.gate_fwd(pooled, w1, b1, w2, b2)
    assert bool((s[:, :2] == 1.0).all()) and bool((s[:, 2:4] == 0.0).all()) and bool(torch.isfinite(s).all())
    got = d.gate_bwd(ds, s, hidden, pooled, w1, w2)
    assert all(bool(torch.isfinite(t).all()) for t in got) and bool((got[4][:4] == 0).all()) and bool((got[3][:4] == 0).all())


@DTYPES
@pytest.mark.parametrize("case", ["c200_r13", "layer4", "layer1", "wide_c4096"])
def test_se_sums_are_deterministic_and_accumulate(pkg, case, T16):
    o = _random_operands(case, T16)
    B, HW, C, R = CASES[case]
    d = _Dev(pkg, T16, B, HW, C, R)
    ref, _ = _gate_reference(o["pooled"], o["w1"], o["b1"], o["w2"], o["b2"], None)
    h32, s32 = ref["hidden"].to(F32), ref["s"].to(F32)
    y16 = F.relu(o["u"] * s32.to(F64)[:, None] + o["sc"]).to(T16).to(F64)
    _, ds1 = d.bwd_reduce(o["dy"], y16, o["u"])
    d.apply_fwd(o["u"], s32, o["sc"])          # an unrelated launch in between
    _, ds2 = d.bwd_reduce(o["dy"], y16, o["u"])
    assert torch.equal(ds1.view(torch.int32), ds2.view(torch.int32))
    args = (o["ds"], s32, h32, o["pooled"], o["w1"], o["w2"])
    first, second = d.gate_bwd(*args), d.gate_bwd(*args)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # accumulate = 1 on a pre-filled target: target + the accumulate = 0 result, one f32 addition
    gen = torch.Generator().manual_seed(9)
    pre = [torch.randn(t.shape, generator=gen) for t in first[1:]]
    acc = d.gate_bwd(*args, accumulate=1, targets=pre)
    assert torch.equal(acc[0].view(torch.int32), first[0].view(torch.int32))
    for name, a, p, f in zip(("dw1", "db1", "dw2", "db2"), acc[1:], pre, first[1:]):
        assert torch.equal(a, p + f), name
    # a non-unit alpha scales the parameter gradients only (powers of two: exactly)
    for alpha in (0.5, 1.0 / 8192.0):
        scaled = d.gate_bwd(*args, alpha=alpha)
        assert torch.equal(scaled[0].view(torch.int32), first[0].view(torch.int32)), "alpha reached dpooled"
        for name, a, f in zip(("dw1", "db1", "dw2", "db2"), scaled[1:], first[1:]):
            assert torch.equal(a, f * alpha), (name, alpha)


@DTYPES
def test_se_refusals_write_nothing(pkg, T16):
    """C = 60, R = 0, R = 257, HW = 0, B = 0 (and C = 0, C = 4104, a batch past grid.y) return MH_ESHAPE, a NULL or misaligned pointer
    MH_EINVAL, and nothing is written; the same calls with valid arguments then succeed."""
    lib = _lib(pkg, T16)
    B, HW, C, R = 2, 6, 64, 8
    f32 = lambda n: torch.full((n,), GUARD32, dtype=F32, device="cuda")
    h16 = lambda: torch.full((B * HW * C + 8,), GUARD16, dtype=T16, device="cuda")
    pooled, w1, b1, w2, b2 = torch.zeros((B, C), device="cuda"), torch.zeros((R, C), device="cuda"), torch.zeros(R, device="cuda"), \
        torch.zeros((C, R), device="cuda"), torch.zeros(C, device="cuda")
    u, sc, dy = (torch.zeros((B * HW, C), dtype=T16, device="cuda") for _ in range(3))
    hidden, s, ds, dpooled, dw1, db1, dw2, db2 = f32(B * R), f32(B * C), f32(B * C), f32(B * C), f32(R * C), f32(R), f32(C * R), f32(C)
    y, g, du = h16(), h16(), h16()
    P = lambda t: t.data_ptr()

    def gate_fwd(B=B, C=C, R=R, pooled=P(pooled), s=P(s)):
        return lib.mh_se_gate_fwd(pooled, P(w1), P(b1), P(w2), P(b2), P(hidden), s, B, C, R, _st())

    def apply_fwd(B=B, HW=HW, C=C, u=P(u), y=P(y), s=P(s)):
        return lib.mh_se_apply_fwd(u, s, P(sc), y, B, HW, C, _st())

    def reduce(B=B, HW=HW, C=C, dy=P(dy), g=P(g), ds=P(ds)):
        return lib.mh_se_apply_bwd_reduce(dy, P(y), P(u), g, ds, B, HW, C, _st())

    def gate_bwd(B=B, C=C, R=R, ds=P(ds), dw1=P(dw1)):
        return lib.mh_se_gate_bwd(ds, P(s), P(hidden), P(pooled), P(w1), P(w2), P(dpooled), dw1, P(db1), P(dw2), P(db2), B, C, R, 1.0, 0, _st())

    def apply_bwd(B=B, HW=HW, C=C, g=P(g), du=P(du), dp=P(dpooled)):
        return lib.mh_se_apply_bwd(g, P(s), dp, du, B, HW, C, _st())

    got = {}
    for what, kw in {"C = 60": dict(C=60), "C = 0": dict(C=0), "C = 4104": dict(C=4104), "B = 0": dict(B=0)}.items():
        got[what] = [(f(**kw), MH_ESHAPE) for f in (gate_fwd, apply_fwd, reduce, gate_bwd, apply_bwd)]
    for what, kw in {"R = 0": dict(R=0), "R = 257": dict(R=257)}.items():
        got[what] = [(f(**kw), MH_ESHAPE) for f in (gate_fwd, gate_bwd)]
    for what, kw in {"HW = 0": dict(HW=0), "B = 65536": dict(B=65536)}.items():
        got[what] = [(f(**kw), MH_ESHAPE) for f in (apply_fwd, reduce, apply_bwd)]
    got["pointers"] = [(gate_fwd(pooled=None), MH_EINVAL), (gate_fwd(s=None), MH_EINVAL), (apply_fwd(u=None), MH_EINVAL), (apply_fwd(y=None), MH_EINVAL),
                       (apply_fwd(y=P(y) + 2), MH_EINVAL), (apply_fwd(s=P(s) + 4), MH_EINVAL), (reduce(dy=None), MH_EINVAL), (reduce(ds=None), MH_EINVAL),
                       (reduce(g=P(g) + 2), MH_EINVAL), (gate_bwd(ds=None), MH_EINVAL), (gate_bwd(dw1=None), MH_EINVAL),
                       (apply_bwd(g=None), MH_EINVAL), (apply_bwd(du=P(du) + 2), MH_EINVAL), (apply_bwd(dp=P(dpooled) + 4), MH_EINVAL)]
    torch.cuda.synchronize()
    for what, pairs in got.items():
        for i, (status, want) in enumerate(pairs):
            assert status == want, f"{what} (call {i}): status {status}, expected {want}"
    for t in (hidden, s, ds, dpooled, dw1, db1, dw2, db2):
        assert bool((t == GUARD32).all()), "a refused call wrote to an output"
    for t in (y, g, du):
        assert bool((t == GUARD16).all()), "a refused call wrote to an output"
    # the same calls with complete, valid arguments (zero operands: hidden = 0, s = 1/2, every gradient 0)
    assert gate_fwd() == 0 and apply_fwd() == 0
    torch.cuda.synchronize()
    assert bool((hidden == 0).all()) and bool((s == 0.5).all()) and bool((y[:B * HW * C] == 0).all()) and bool((y[B * HW * C:] == GUARD16).all())
    assert reduce() == 0 and gate_bwd() == 0 and apply_bwd() == 0
    torch.cuda.synchronize()
    for t in (ds, dpooled, dw1, db1, dw2, db2, g[:B * HW * C], du[:B * HW * C]):
        assert bool((t == 0).all())
    assert bool((g[B * HW * C:] == GUARD16).all()) and bool((du[B * HW * C:] == GUARD16).all())


# ---------------------------------------------------------------------------------------------------------------------
# B. the tower
# ---------------------------------------------------------------------------------------------------------------------

BARS = {"fp16": (1e-2, 5e-2), "bf16": (6e-2, 1.5e-1)}          # (ftol, gtol) of tests/test_resnet_gpu.py's tower test
LAYERS, SIZE, NUM_CLASSES, GROUPS = (1, 1, 1, 1), 64, 10, 32


class _RoundSTE(torch.autograd.Function):
    """x -> x rounded to the 16-bit storage type (straight-through); `gscale` > 0: an ACTIVATION, whose gradient the tower stores in 16 bits as
    well (scaled by `gscale`); 0: a weight, whose gradient is produced in f32.  (tests/test_resnext_gpu.py's, restated.)"""

    @staticmethod
    def forward(ctx, x, dtype, gscale):
        ctx.dtype, ctx.gscale = dtype, gscale
        return x.to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        if ctx.gscale:
            g = (g * ctx.gscale).to(ctx.dtype).to(g.dtype) / ctx.gscale
        return g, None, None


def _ref_features(p, st, image, layers, training, storage, groups=GROUPS):
    """tests/test_resnext_gpu.py's composition (a bottleneck ResNet with a grouped conv2 over a torchvision-keyed dict, in the arithmetic of
    its operands; `storage`: the tower's 16-bit storage points, straight-through) extended by the SE block: u = q(bn3(.)) is stored, the
    squeeze, the two layers and the gate s stay in the operands' arithmetic (f32 on the device) with unrounded fc1 / fc2 parameters, and
    out = q(relu(u * s + shortcut)).  `st`: running statistics, updated in place when training."""
    gs = 8192.0 if storage == F16 else 1.0
    q = (lambda t: _RoundSTE.apply(t, storage, gs)) if storage is not None else (lambda t: t)
    qw = (lambda t: _RoundSTE.apply(t, storage, 0.0)) if storage is not None else (lambda t: t)

    def conv(x, w, **kw):
        return q(F.conv2d(q(x), qw(w), **kw))

    def bn(x, pfx):
        return F.batch_norm(x, st[pfx + ".running_mean"], st[pfx + ".running_var"], p[pfx + ".weight"], p[pfx + ".bias"], training, 0.1, 1e-5)

    x = q(F.relu(bn(conv(image, p["conv1.weight"], stride=2, padding=3), "bn1")))
    x = F.max_pool2d(x, 3, 2, 1)
    for li, (n, stride) in enumerate(zip(layers, (1, 2, 2, 2)), 1):
        for bi in range(n):
            L = f"layer{li}.{bi}."
            s = stride if bi == 0 else 1
            o = q(F.relu(bn(conv(x, p[L + "conv1.weight"]), L + "bn1")))
            o = q(F.relu(bn(conv(o, p[L + "conv2.weight"], stride=s, padding=1, groups=groups), L + "bn2")))
            u = q(bn(conv(o, p[L + "conv3.weight"]), L + "bn3"))
            idn = x
            if (L + "downsample.0.weight") in p:
                idn = q(bn(conv(x, p[L + "downsample.0.weight"], stride=s), L + "downsample.1"))
            hidden = F.relu(F.conv2d(u.mean(dim=(2, 3), keepdim=True), p[L + "se.fc1.weight"], p[L + "se.fc1.bias"]))
            gate = torch.sigmoid(F.conv2d(hidden, p[L + "se.fc2.weight"], p[L + "se.fc2.bias"]))
            x = q(F.relu(u * gate + idn))
    return x.mean(dim=(2, 3))


def _split_state(sd):
    p = {k: v.detach().cpu().to(F64) for k, v in sd.items() if "running_" not in k and "num_batches" not in k}
    st = {k: v.detach().cpu().to(F64).clone() for k, v in sd.items() if "running_" in k}
    return p, st


# The seed rule of tests/test_resnext_gpu.py: picked on the CPU from the reference alone -- the smallest seed >= 11 for which the
# storage-rounded reference evaluated in float32 stays within 1.25 x deviation + 0.01 for every tensor and both dtypes; the test asserts
# it at the bar (1.5 x) before the GPU is touched.  SEEDS_REJECTED lists the seeds below SEED that did not qualify.
SEED = 13
SEEDS_REJECTED = (11, 12)          # fp16: layer4.0.conv2.weight (11), layer3.0.bn3.bias and layer3.0.se.fc1.* (12) outside 1.25 x + 0.01 in float32


def _gradient_misses(grads, ref_grads, q_grads, factor=1.5):
    out = []
    for name, ref in ref_grads.items():
        den = float(ref.norm()) + 1e-12
        rel, sens = float((grads[name].to(F64) - ref).norm()) / den, float((q_grads[name] - ref).norm()) / den
        if rel > factor * sens + 0.01:
            out.append((name, round(rel, 4), round(sens, 4)))
    return out


@lru_cache(maxsize=None)
def _tower_reference(pkg, dtype, seed=SEED):
    T16 = F16 if dtype == "fp16" else BF16
    net = pkg.SEResNeXt50_32x4d(num_classes=NUM_CLASSES, compute_dtype=dtype, layers=LAYERS, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for n, prm in net.named_parameters():          # BatchNorm affine parameters and the SE biases off their 1 / 0 (/ small) defaults
        if prm.dim() == 1 and not n.startswith("fc."):
            prm.data = (torch.rand(prm.shape, generator=g) + 0.5) if n.endswith("weight") else torch.randn(prm.shape, generator=g) * 0.2
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    image = torch.randn((2, 3, SIZE, SIZE), generator=g)
    labels = torch.tensor([3, 8])
    p, st0 = _split_state(sd)

    def run(storage, arith=F64):
        leaves = {k: v.detach().to(arith).clone().requires_grad_(True) for k, v in p.items()}
        st = {k: v.to(arith).clone() for k, v in st0.items()}
        feats = _ref_features(leaves, st, image.to(arith), LAYERS, True, storage)
        logits = F.linear(feats, leaves["fc.weight"], leaves["fc.bias"])
        F.cross_entropy(logits, labels).backward()
        return logits.detach(), {k: v.grad for k, v in leaves.items()}, st
    return dict(sd=sd, image=image, labels=labels, plain=run(None), rounded=run(T16), rounded_f32=run(T16, F32), T16=T16)


def seed_qualifies(pkg, seed, factor=1.25):
    """the seed rule, on the CPU: no tensor of either dtype outside factor x deviation + 0.01 in the float32 evaluation"""
    for dtype in ("fp16", "bf16"):
        r = _tower_reference(pkg, dtype, seed)
        if _gradient_misses(r["rounded_f32"][1], r["plain"][1], r["rounded"][1], factor):
            return False
    return True


def _record_launches(monkeypatch, pkg, lib):
    """every mh_* entry point of `lib` wrapped to append its name to the returned list (as tests/test_basic_resnet_gpu.py::_count_pairs
    wraps one)"""
    names = []
    for name in pkg._lib.EXPORTED_SYMBOLS:
        real = getattr(lib, name)

        def wrapped(*a, _real=real, _name=name):
            names.append(_name)
            return _real(*a)
        monkeypatch.setattr(lib, name, wrapped)
    return names


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_seresnext_forward_backward_matches_float64(pkg, monkeypatch, dtype):
    ftol, gtol = BARS[dtype]
    r = _tower_reference(pkg, dtype)
    ref_logits, ref_grads, _ = r["plain"]
    q_logits, q_grads, q_st = r["rounded"]
    assert not _gradient_misses(r["rounded_f32"][1], ref_grads, q_grads), "the reference misses its own bar in float32: SEED is no usable input"
    net = pkg.SEResNeXt50_32x4d(num_classes=NUM_CLASSES, compute_dtype=dtype, layers=LAYERS)
    net.load_state_dict(r["sd"])
    net.cuda().train()
    names = _record_launches(monkeypatch, pkg, pkg._lib.load(dtype))
    logits = net(r["image"].cuda())
    pkg.CrossEntropyLoss()(logits, r["labels"].cuda()).backward()
    torch.cuda.synchronize()
    # one of each mh_se_* entry point per block and step, the squeeze per block and the tower's own pool
    assert {n: names.count(n) for n in SE_ENTRY_POINTS} == {n: 4 for n in SE_ENTRY_POINTS}, names
    assert names.count("mh_avgpool_fwd") == 5 and names.count("mh_add_h16") == 4          # (every block above an SE block adds its two branches)
    got_logits = logits.detach().cpu().to(F64)
    err, errq = float((got_logits - ref_logits).abs().max()), float((got_logits - q_logits).abs().max())
    sens_f = float((q_logits - ref_logits).abs().max())
    tag = f"[seresnext50_32x4d 1111@64 {dtype}]"
    parity_log(f"{tag} max |logit - float64| = {err:.3e} (vs the storage-rounded reference {errq:.3e}; storage rounding alone {sens_f:.3e}; "
               f"|logit| max {float(ref_logits.abs().max()):.3f})")
    assert err < ftol * max(1.0, float(ref_logits.abs().max())) and errq < 0.5 * ftol
    worst, worst_n, fails = ("", 0.0, 0.0), ("", 0.0), []
    for name, prm in net.named_parameters():
        got = prm.grad.detach().cpu().to(F64)
        den = float(ref_grads[name].norm()) + 1e-12
        rel = float((got - ref_grads[name]).norm()) / den
        sens = float((q_grads[name] - ref_grads[name]).norm()) / den
        nq = float(q_grads[name].norm())
        dn = abs(float(got.norm()) - nq) / (nq + 1e-30)
        if rel > worst[1]:
            worst = (name, rel, sens)
        if dn > worst_n[1]:
            worst_n = (name, dn)
        if rel > 1.5 * sens + 0.01:
            fails.append(f"{name}: |hip - float64| / |float64| = {rel:.3f}, storage rounding alone gives {sens:.3f}")
        if abs(float(got.norm()) - nq) > gtol * nq + 1e-7:
            fails.append(f"{name}: gradient norm off the storage-rounded reference's by {dn:.3f} (bar {gtol})")
        if ".se." in name:
            assert float(got.abs().max()) > 0, f"{name} received no gradient"
    parity_log(f"{tag} worst gradient deviation from float64 {worst[1]:.3f} ({worst[0]}; 16-bit storage alone: {worst[2]:.3f}); "
               f"worst norm deviation from the storage-rounded reference {worst_n[1]:.3f} ({worst_n[0]})")
    assert not fails, fails[:6]
    assert sum(".se." in n for n, _ in net.named_parameters()) == 16
    sd = net.state_dict()
    for k, v in q_st.items():          # running statistics advance as nn.BatchNorm2d's (F.batch_norm's) do
        bar = (2e-3 if k.endswith("running_mean") else 2e-2) * max(1.0, float(v.abs().max()))
        assert float((sd[k].cpu().to(F64) - v).abs().max()) < bar, k
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked")) and int(sd["layer4.0.bn3.num_batches_tracked"]) == 1
    net.eval()          # eval mode: the running statistics; features against the float64 composition with the same statistics
    with torch.no_grad():
        feats = net.features(r["image"].cuda()).cpu().to(F64)
    p, st = _split_state(sd)
    ref_e = _ref_features(p, st, r["image"].to(F64), LAYERS, False, None)
    q_e = _ref_features(p, st, r["image"].to(F64), LAYERS, False, r["T16"])
    e, eq = float((feats - ref_e).abs().max()), float((feats - q_e).abs().max())
    parity_log(f"{tag} eval features: max |f - float64| = {e:.3e} (vs storage-rounded {eq:.3e}; |f| max {float(ref_e.abs().max()):.3f})")
    assert feats.shape == (2, 2048) and e < ftol * max(1.0, float(ref_e.abs().max())) and eq < 0.5 * ftol
    assert all(int(v) == 1 for k, v in net.state_dict().items() if k.endswith("num_batches_tracked"))


def test_seresnext_gradients_accumulate_in_place_like_autograd(pkg):
    torch.manual_seed(1)
    net = pkg.SEResNeXt50_32x4d(num_classes=10, compute_dtype="fp16", layers=LAYERS).cuda().train()
    g = torch.Generator().manual_seed(2)
    image = torch.randn((4, 3, 64, 64), generator=g).cuda()
    labels = torch.tensor([1, 7, 3, 3]).cuda()
    ce = pkg.CrossEntropyLoss()
    ce(net(image), labels).backward()
    first = {n: p.grad.clone() for n, p in net.named_parameters()}
    ce(net(image), labels).backward()          # .grad exists now: the in-place path (mh_se_gate_bwd with accumulate = 1 for the gates)
    torch.cuda.synchronize()
    assert sum(".se." in n for n in first) == 16
    for n, p in net.named_parameters():
        ref = 2.0 * first[n]
        assert float(ref.abs().max()) > 0, n
        assert float((p.grad - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-12, n
    assert int(net.bn1.num_batches_tracked) == 2 and int(net.layer4[0].bn3.num_batches_tracked) == 2


def test_seresnext_classifier_step_moves_every_parameter(pkg):
    torch.manual_seed(0)
    model = pkg.ResNetClassifier(num_labels=2, compute_dtype="fp16", arch="seresnext50_32x4d", layers=LAYERS).cuda()
    assert type(model.resnet) is pkg.SEResNeXt50_32x4d
    pkg.flatten_parameters(model)
    model.train()
    g = torch.Generator().manual_seed(3)
    batch = {"pixel_values": torch.randn((8, 3, 64, 64), generator=g).cuda(), "labels": torch.tensor([0, 1, 1, 0, 1, 0, 0, 1]).cuda()}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = pkg.Adam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    loss, logits = model(**batch)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert logits.shape == (8, 2) and np.isfinite(float(loss.detach()))
    assert sum(".se." in n for n in before) == 16
    for n, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[n]), n


def test_kevin_model_over_seresnext(pkg):
    tc = pkg.TextConfig(vocab_size=600, hidden=128, layers=1, heads=2, intermediate=256, max_position=64)
    cc = pkg.TextConfig(vocab_size=500, hidden=128, layers=1, heads=2, intermediate=256, max_position=64)
    model = pkg.KevinMultimodalClassifier("concatenation", text=tc, image="seresnext50_32x4d", caption=cc, proj=128, compute_dtype="fp16", seed=1,
                                          resnet_layers=LAYERS).cuda().train()
    assert type(model.image_model) is pkg.SEResNeXt50_32x4d and model.image_fine_tune[0].in_features == 2048
    n, S = 4, 16
    g = torch.Generator().manual_seed(5)
    text, cap = torch.randint(5, 600, (n, S), generator=g), torch.randint(5, 500, (n, S), generator=g)
    mask = (torch.arange(S)[None] < torch.randint(4, S + 1, (n,), generator=g)[:, None]).long()
    image = torch.randn((n, 3, 64, 64), generator=g)
    out = model(*[t.cuda() for t in (text * mask, image, mask, cap * mask, mask)])
    pkg.SigmoidFocalLoss()(out, torch.tensor([0.0, 1.0, 1.0, 0.0]).cuda()).backward()
    torch.cuda.synchronize()
    assert out.shape == (n,) and bool(torch.isfinite(out).all())
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    groups = model.get_params(1e-3)
    image_ids = {id(p) for p in groups[2]["params"]}
    assert all(id(p) in image_ids for p in model.image_model.parameters())


class _TorchBH(nn.Module):
    """SEResNeXt50_32x4d_BH's head written with torch.nn (example_scripts/Untitled-2.py:164-179,194-207), over given features"""

    def __init__(self, D):
        super().__init__()
        self.fea_bn = nn.BatchNorm1d(D)
        self.fea_bn.bias.requires_grad_(False)
        self.fc = nn.Sequential(nn.Linear(D, 2))
        self.s = 1

    def forward(self, fea):
        fea = self.fea_bn(fea)
        fea = torch.div(fea, torch.norm(fea, 2, 1, True))
        return self.fc(fea) * self.s


def test_seresnext_binary_head_model_against_torch_float64(pkg):
    """The head (fea_bn -> l2_norm -> Linear -> x s) in f32 on the device against torch.nn in float64 over the tower's own features, with the
    bar of tests/test_resnext_gpu.py's twin: every op is a sum of at most D = 2048 f32 terms (error <= D 2^-24 of sum|terms|); six such ops
    are chained (three forward, three backward) and at B = 4 the BatchNorm's 1 / sigma amplifies a feature's error by up to ~sqrt(B): bar
    6 * 2 * D 2^-24 = 3e-3 of a tensor's largest entry.  Then the whole model, tower + head, in one forward / backward."""
    model = pkg.SEResNeXt50_32x4d_BH(compute_dtype="fp16", layers=LAYERS, seed=3).cuda().train()
    g = torch.Generator().manual_seed(8)
    x = torch.randn((4, 3, 64, 64), generator=g).cuda()
    labels = torch.tensor([0, 1, 1, 0])
    with torch.no_grad():
        model.eval()
        feats = model.net.features(x)            # eval: the same features for both evaluations below
    D = feats.shape[1]
    ref = _TorchBH(D).double().train()
    ref.load_state_dict({"fea_bn." + k: v.cpu().double() for k, v in model.fea_bn.state_dict().items()}
                        | {"fc.0." + k: v.cpu().double() for k, v in model.binary_head.fc[0].state_dict().items()})
    f64 = feats.cpu().double().requires_grad_(True)
    ref_logits = ref(f64)
    F.cross_entropy(ref_logits, labels).backward()
    model.fea_bn.train(), model.binary_head.train()
    fd = feats.clone().requires_grad_(True)
    logits = model.binary_head(model.fea_bn(fd))
    pkg.CrossEntropyLoss()(logits, labels.cuda()).backward()
    torch.cuda.synchronize()
    bar = 12 * D * 2.0 ** -24

    def close(what, got, want):
        err, size = float((got.detach().cpu().double() - want).abs().max()), float(want.abs().max())
        parity_log(f"[seresnext50_32x4d_BH] {what}: max error {err:.3e} of max |ref| {size:.3e} (bar {bar:.1e} of it)")
        assert err <= bar * size, what
    assert logits.shape == (4, 2)
    close("logits", logits, ref_logits.detach())
    close("d features", fd.grad, f64.grad)
    close("fea_bn.weight.grad", model.fea_bn.weight.grad, ref.fea_bn.weight.grad)
    close("binary_head.fc.0.weight.grad", model.binary_head.fc[0].weight.grad, ref.fc[0].weight.grad)
    close("binary_head.fc.0.bias.grad", model.binary_head.fc[0].bias.grad, ref.fc[0].bias.grad)
    close("fea_bn.running_mean", model.fea_bn.running_mean, ref.fea_bn.running_mean)
    assert model.fea_bn.bias.grad is None and ref.fea_bn.bias.grad is None
    model.train()
    model.zero_grad()
    out = model(x)
    pkg.CrossEntropyLoss()(out, labels.cuda()).backward()
    torch.cuda.synchronize()
    assert out.shape == (4, 2) and bool(torch.isfinite(out).all()) and model.fea_bn.bias.grad is None
    for name, p in model.named_parameters():
        if name != "fea_bn.bias":          # (the frozen bias)
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name


def test_resnext_step_is_unchanged_and_launches_no_se_kernel(pkg, monkeypatch):
    """A fixed seed, ResNeXt50_32x4d(layers=(1, 1, 1, 1)): the logits and every gradient of a step whose launches are recorded (every mh_*
    entry point wrapped) are bit for bit those of the same step run plainly, and the recorded list holds no mh_se_* name, one
    mh_avgpool_fwd (the tower's own pool) and one mh_add_h16 (the first block's, above the max pool) -- every conv1 above a block still takes
    the block-out epilogue."""
    def step(record):
        net = pkg.ResNeXt50_32x4d(num_classes=NUM_CLASSES, compute_dtype="fp16", layers=LAYERS, seed=5).cuda().train()
        names = _record_launches(monkeypatch, pkg, pkg._lib.load("fp16")) if record else None
        g = torch.Generator().manual_seed(6)
        image, labels = torch.randn((2, 3, SIZE, SIZE), generator=g).cuda(), torch.tensor([3, 8]).cuda()
        logits = net(image)
        pkg.CrossEntropyLoss()(logits, labels).backward()
        torch.cuda.synchronize()
        return logits.detach().cpu(), {n: p.grad.detach().cpu() for n, p in net.named_parameters()}, names
    plain_logits, plain_grads, _ = step(False)
    logits, grads, names = step(True)
    assert torch.equal(plain_logits, logits)
    for n, gr in grads.items():
        assert torch.equal(gr.view(torch.int32), plain_grads[n].view(torch.int32)), n
    assert names and not [n for n in names if n.startswith("mh_se_")], names
    assert names.count("mh_avgpool_fwd") == 1 and names.count("mh_add_h16") == 1 and names.count("mh_gconv_fwd") == 4
    assert names.count("mh_conv_dgrad") >= 3          # (the three block-out conv1 among them)
