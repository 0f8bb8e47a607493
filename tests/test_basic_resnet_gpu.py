"""The basic-block ResNet tower on the MI355X.

Part A -- ``mh_conv_dgrad_pair`` alone: dx = dgrad(k x k / 2) + dgrad(1x1 / 2) of two convolutions over the same input, one launch.
  Reference: float64 autograd of both ``F.conv2d`` on the CPU from the same 16-bit tensors, summed in float64.  The tolerance rule is
  tests/test_resnet_paths_gpu.py's, restated: a stored 16-bit value within 1 ulp + 1e-5 x (sum of |terms|) of the float64 value, a
  BatchNorm partial within 1e-5 x (sum of |terms|); where the ReLU mask is recomputed from z, an element whose pre-activation lies
  inside one ulp of zero is a rounding call and takes the kernel's decision (at most 1 % of a tensor, asserted on the reference alone).
  Exactness leg: integer-valued operands whose sums are exact in f32 -- the result is ``F.conv2d``'s autograd bit for bit.
Part B -- ``ResNet18`` (one or two blocks per stage, true widths) forward + backward against a float64 ``F.conv2d / F.batch_norm``
  composition written here, with the tower's 16-bit storage rounding inserted (straight-through) where the tower stores 16 bits (forward
  activations and packed weights, and the activation gradients of its 16-bit gradient stream); metric
  and bars of tests/test_resnet_gpu.py::test_resnet_tower_forward_backward_matches_the_oracle (ftol / gtol per dtype from there; a
  gradient within 1.5 x the storage-rounded-vs-plain-float64 deviation + 0.01).  ``TowerOptions.pair_dgrad`` on / off: the same checks,
  and the number of ``mh_conv_dgrad_pair`` launches.  Then the classifier and Kevin's three-tower model over the new tower."""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from conftest import parity_log

pytestmark = pytest.mark.gpu
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("T16", [F16, BF16], ids=["fp16", "bf16"])
MANT = {F16: 10, BF16: 7}
EMIN = {F16: -14, BF16: -126}
TOL_SUM = 1e-5
BN_EPS = 1e-5
MH_EINVAL, MH_ESHAPE = 1, 2


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


def _r16(t, T16):
    return t.to(T16).to(F64)


def _ulp(ref, T16):
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** EMIN[T16]))
    return torch.pow(2.0, (e - 1 - MANT[T16]).to(F64))


def _cpu(t):
    return t.detach().cpu().to(F64)


def _dev(t64, T16):
    return t64.to(T16).cuda().contiguous()


def _rand(shape, g, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=g, dtype=F64) * scale + shift


def _check_stored(what, got, ref, T16, terms=None):
    """16-bit outputs: |got - ref| <= ulp(ref) (+ TOL_SUM * terms).  Returns the worst error as a fraction of the bar."""
    got = _cpu(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
    tol = _ulp(ref, T16) + (0.0 if terms is None else TOL_SUM * terms)
    frac = (got - ref).abs() / tol
    worst = float(frac.max()) if frac.numel() else 0.0
    if worst > 1.0:
        i = int(frac.argmax())
        raise AssertionError(f"{what}: {int((frac > 1.0).sum())}/{frac.numel()} off by more than the bar; worst {worst:.3g} x bar "
                             f"(ref {float(ref.flatten()[i]):.6g}, got {float(got.flatten()[i]):.6g}, bar {float(tol.flatten()[i]):.3g})")
    return worst


def _check_sum(what, got, ref, terms, tol=TOL_SUM):
    """sums: |got - ref| <= tol * (sum of |terms|).  Returns the worst error relative to the sum of |terms|."""
    got = _cpu(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
    err = (got - ref).abs()
    rel = err / terms.clamp_min(1e-30)
    worst = float(rel.max()) if rel.numel() else 0.0
    if (err > tol * terms + 1e-30).any():
        i = int(rel.argmax())
        raise AssertionError(f"{what}: worst {worst:.3g} of sum|terms| (bar {tol:.1g}; ref {float(ref.flatten()[i]):.6g}, "
                             f"got {float(got.flatten()[i]):.6g})")
    return worst


def _nhwc(x4):
    return x4.permute(0, 2, 3, 1).reshape(-1, x4.shape[1])


def _geom(pkg, B, H, W, C, k, s, p, Cout, ldk):
    g = pkg._lib.MhConvGeom()
    g.B, g.H, g.W, g.C, g.KH, g.KW, g.stride, g.pad, g.Cout, g.ldk = B, H, W, C, k, k, s, p, Cout, ldk
    return g


def _pack(pkg, lib, w64, ldk, T16):
    """w64 holds 16-bit values already: the pack is exact"""
    Cout, Cin, k, _ = w64.shape
    wd = w64.to(F32).cuda().contiguous()
    wk = torch.empty((Cout, ldk), dtype=T16, device="cuda")
    pkg._lib.check(lib.mh_conv_weight_pack(wd.data_ptr(), wk.data_ptr(), Cout, Cin, k, k, Cin, ldk, _st()), "pack")
    return wk


# ---------------------------------------------------------------------------------------------------------------------
# A. mh_conv_dgrad_pair
# ---------------------------------------------------------------------------------------------------------------------

# (B, H, W, C, Cout, Cout2): 3x3 / 2 / pad 1 + 1x1 / 2 / pad 0
PAIR_GEOMS = {
    "ragged_m": (2, 8, 8, 64, 128, 128),          # 32 rows per class: one ragged M tile each, half-empty N tile
    "three_tiles": (3, 20, 20, 128, 256, 256),    # 300 rows per class = 3 tiles, the last ragged; 4 K tiles in the second segment
    "tiny": (1, 4, 2, 64, 64, 64),                # 2 rows per class; Cout2 at its minimum (one K tile)
    "ragged_n": (2, 12, 12, 192, 128, 128),       # 2 N tiles, the second half-empty
    "cout2_differs": (2, 10, 6, 64, 64, 192),     # Cout2 != Cout: 1 K tile of the centre tap + 3 of the second segment
}
# the BatchNorm epilogue as the tower uses it: (addend, y_mask, relu)
BN_FORMS = {"relu": (False, False, 1), "block_out": (True, True, 1), "y_mask": (False, True, 1), "plain": (False, False, 0)}
MASK_SKIP_MAX = 0.01


def _pair_tiles(B, H, W):
    """the partial column (tile) of every dx row: 128-row tiles per parity class, classes in (ph, pw) order"""
    Hh, Wh = H // 2, W // 2
    per = (B * Hh * Wh + 127) // 128
    b = torch.arange(B)[:, None, None]
    h = torch.arange(H)[None, :, None]
    w = torch.arange(W)[None, None, :]
    cls = (h % 2) * 2 + (w % 2)
    r = (b * Hh + h // 2) * Wh + w // 2
    return (cls * per + r // 128).reshape(-1), 4 * per


@lru_cache(maxsize=None)
def _pair_reference(case, T16):
    """float64, CPU only: operands (16-bit values), the summed input gradient, the sum of |terms|, and the BatchNorm below"""
    B, H, W, C, Cout, Cout2 = PAIR_GEOMS[case]
    g = torch.Generator().manual_seed(900 + 7 * list(PAIR_GEOMS).index(case) + (0 if T16 == F16 else 1))
    Ho, Wo = H // 2, W // 2
    w = _r16(_rand((Cout, C, 3, 3), g, 1.0 / math.sqrt(Cout * 9 / 4)), T16)
    w2 = _r16(_rand((Cout2, C, 1, 1), g, 1.0 / math.sqrt(Cout2)), T16)
    dy = _r16(_rand((B, Cout, Ho, Wo), g), T16)
    dy2 = _r16(_rand((B, Cout2, Ho, Wo), g), T16)

    def both(w, w2, dy, dy2):
        x = torch.zeros((B, C, H, W), dtype=F64, requires_grad=True)
        ((F.conv2d(x, w, stride=2, padding=1) * dy).sum() + (F.conv2d(x, w2, stride=2) * dy2).sum()).backward()
        return _nhwc(x.grad)
    ref, terms = both(w, w2, dy, dy2), both(w.abs(), w2.abs(), dy.abs(), dy2.abs())
    Mi = B * H * W
    z = _r16(_rand((Mi, C), g, 1.3, 0.2), T16)
    mu = z.mean(0)
    mean, rstd = mu.to(F32), (1.0 / torch.sqrt(((z - mu) ** 2).mean(0) + BN_EPS)).to(F32)
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).to(F32).to(F64)
    beta = _rand(C, g, 0.5).to(F32).to(F64)
    xh = (z - mean.to(F64)) * rstd.to(F64)
    v = xh * gamma + beta
    y_mask = _r16((v + _r16(_rand((Mi, C), g), T16)).clamp_min(0.0), T16)           # the block's stored output relu(bn(z) + residual)
    addend = _r16(_rand((Mi, C), g), T16)
    unsure = v.abs() <= _ulp((xh * gamma).abs() + beta.abs(), T16)
    return dict(w=w, w2=w2, dy=dy, dy2=dy2, ref=ref, terms=terms, z=z, mean=mean, rstd=rstd, gamma=gamma, beta=beta, xh=xh, v=v,
                y_mask=y_mask, addend=addend, unsure=unsure)


def _bn_bwd_ref(z, gamma, gp):
    zr = z.clone().requires_grad_(True)
    ga = gamma.clone().requires_grad_(True)
    be = torch.zeros_like(gamma, requires_grad=True)
    mu = zr.mean(0)
    var = ((zr - mu) ** 2).mean(0)
    ((zr - mu) / torch.sqrt(var + BN_EPS) * ga + be).backward(gp)
    return zr.grad, ga.grad, be.grad


@DTYPES
@pytest.mark.parametrize("case", list(PAIR_GEOMS))
def test_dgrad_pair_against_float64(pkg, case, T16):
    lib = _lib(pkg, T16)
    B, H, W, C, Cout, Cout2 = PAIR_GEOMS[case]
    r = _pair_reference(case, T16)
    skipped = float(r["unsure"].double().mean())
    assert skipped <= MASK_SKIP_MAX, f"{case}: the mask rule would skip {skipped:.2%} of the tensor"
    Mi, ldk = B * H * W, 9 * C
    geom = _geom(pkg, B, H, W, C, 3, 2, 1, Cout, ldk)
    wk, wk2 = _pack(pkg, lib, r["w"], ldk, T16), _pack(pkg, lib, r["w2"], C, T16)
    dyd, dy2d = _dev(_nhwc(r["dy"]), T16), _dev(_nhwc(r["dy2"]), T16)
    tiles, nblk = _pair_tiles(B, H, W)
    assert nblk == 4 * ((B * (H // 2) * (W // 2) + 127) // 128)
    CANARY = 16

    def run(bn, what):
        buf = torch.full((Mi + CANARY, C), 7.0, dtype=T16, device="cuda")
        pkg._lib.check(lib.mh_conv_dgrad_pair(dyd.data_ptr(), wk.data_ptr(), dy2d.data_ptr(), wk2.data_ptr(), C, Cout2, buf.data_ptr(), geom, bn,
                                              _st()), what)
        torch.cuda.synchronize()
        assert bool((buf[Mi:] == 7.0).all()), f"{what}: wrote past dx"
        return buf[:Mi]

    tag = f"dgrad_pair {case} {_name(T16)}"
    plain = run(None, tag)
    errs = {"plain": _check_stored(tag, plain, r["ref"], T16, terms=r["terms"])}
    D = _cpu(plain)
    z, xh, gamma, mean, rstd = r["z"], r["xh"], r["gamma"], r["mean"], r["rstd"]
    zd, md, rsd, gd, bd = _dev(z, T16), mean.cuda(), rstd.cuda(), gamma.to(F32).cuda(), r["beta"].to(F32).cuda()
    ymd, add_d = _dev(r["y_mask"], T16), _dev(r["addend"], T16)
    for form, (add, ym, relu) in BN_FORMS.items():
        ftag = f"{tag} bn={form}"
        f = pkg._lib.MhConvBnBwd()
        part = torch.full((2 * C * nblk + 256,), 12345.0, dtype=F32, device="cuda")
        f.z, f.mean, f.rstd, f.gamma, f.beta, f.part, f.relu = zd.data_ptr(), md.data_ptr(), rsd.data_ptr(), gd.data_ptr(), bd.data_ptr(), part.data_ptr(), relu
        f.addend = add_d.data_ptr() if add else None
        f.y_mask = ymd.data_ptr() if ym else None
        gm = run(f, ftag)
        assert bool((part[2 * C * nblk:] == 12345.0).all()), f"{ftag}: wrote past part"
        part = part[:2 * C * nblk].view(2, C, nblk)
        gsum = _r16(D + r["addend"], T16) if add else D           # the stored input gradient, then mh_add_h16's rounding of the sum
        if not relu:
            keep, unsure = torch.ones_like(z, dtype=torch.bool), torch.zeros_like(z, dtype=torch.bool)
        elif ym:
            keep, unsure = r["y_mask"] > 0, torch.zeros_like(z, dtype=torch.bool)
        else:
            keep, unsure = _r16(r["v"], T16) > 0, r["unsure"]
        gp = torch.where(keep, gsum, torch.zeros_like(gsum))
        gp = torch.where(unsure, _cpu(gm), gp)                    # a rounding call either way: the kernel's decision
        errs[f"{form}.masked"] = _check_stored(f"{ftag} masked gradient", gm, gp, T16)
        s0 = torch.zeros((nblk, C), dtype=F64).index_add_(0, tiles, gp)
        s1 = torch.zeros((nblk, C), dtype=F64).index_add_(0, tiles, gp * xh)
        a0 = torch.zeros((nblk, C), dtype=F64).index_add_(0, tiles, gp.abs())
        a1 = torch.zeros((nblk, C), dtype=F64).index_add_(0, tiles, (gp * xh).abs())
        errs[f"{form}.part"] = max(_check_sum(f"{ftag} part sum g'", part[0], s0.t(), a0.t()),
                                   _check_sum(f"{ftag} part sum g' xhat", part[1], s1.t(), a1.t()))
        # ... and the partials feed mh_bn2d_bwd_parts
        dx = torch.full((Mi, C), 7.0, dtype=T16, device="cuda")
        dg, db = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
        sums = torch.full((2, C), float("nan"), device="cuda")
        pkg._lib.check(lib.mh_bn2d_bwd_parts(gm.data_ptr(), zd.data_ptr(), part.data_ptr(), nblk, gd.data_ptr(), md.data_ptr(), rsd.data_ptr(),
                                             dx.data_ptr(), dg.data_ptr(), db.data_ptr(), sums.data_ptr(), Mi, C, 0, 1.0, _st()), "mh_bn2d_bwd_parts")
        torch.cuda.synchronize()
        dx_ref, dg_ref, db_ref = _bn_bwd_ref(z, gamma, gp)
        s_abs, q_abs = gp.abs().sum(0), (gp * xh).abs().sum(0)
        terms = gamma.abs() * rstd.to(F64) * (gp.abs() + s_abs / Mi + xh.abs() * q_abs / Mi)
        errs[f"{form}.bn_dx"] = _check_stored(f"{ftag} bn dx", dx, dx_ref, T16, terms=terms)
        errs[f"{form}.dgamma"] = _check_sum(f"{ftag} dgamma", dg, dg_ref, q_abs)
        errs[f"{form}.dbeta"] = _check_sum(f"{ftag} dbeta", db, db_ref, s_abs)
    parity_log(f"[{tag}] mask rule skips {skipped:.3%}; worst error / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))


@DTYPES
def test_dgrad_pair_is_exact_on_integers(pkg, T16):
    """Integer operands, |sum| <= 3 * 2 * (4 * 128 + 192) < 2^24: every f32 partial sum is exact, so the stored value is the rounding
    of the exact sum -- F.conv2d's autograd in float64, rounded once, bit for bit."""
    lib = _lib(pkg, T16)
    B, H, W, C, Cout, Cout2 = 2, 12, 10, 192, 128, 192
    g = torch.Generator().manual_seed(77)
    ri = lambda shape, a: torch.randint(-a, a + 1, shape, generator=g).to(F64)
    w, w2, dy, dy2 = ri((Cout, C, 3, 3), 2), ri((Cout2, C, 1, 1), 2), ri((B, Cout, H // 2, W // 2), 3), ri((B, Cout2, H // 2, W // 2), 3)
    x = torch.zeros((B, C, H, W), dtype=F64, requires_grad=True)
    ((F.conv2d(x, w, stride=2, padding=1) * dy).sum() + (F.conv2d(x, w2, stride=2) * dy2).sum()).backward()
    want = _nhwc(x.grad).to(T16)
    wk, wk2 = _pack(pkg, lib, w, 9 * C, T16), _pack(pkg, lib, w2, C, T16)
    dyd, dy2d = _dev(_nhwc(dy), T16), _dev(_nhwc(dy2), T16)
    dx = torch.full((B * H * W, C), 7.0, dtype=T16, device="cuda")
    pkg._lib.check(lib.mh_conv_dgrad_pair(dyd.data_ptr(), wk.data_ptr(), dy2d.data_ptr(), wk2.data_ptr(), C, Cout2, dx.data_ptr(),
                                          _geom(pkg, B, H, W, C, 3, 2, 1, Cout, 9 * C), None, _st()), "mh_conv_dgrad_pair")
    torch.cuda.synchronize()
    assert float(want.float().abs().max()) > 64          # (not a trivially small problem)
    assert torch.equal(dx.cpu().view(torch.int16), want.view(torch.int16))


@DTYPES
def test_dgrad_pair_refusals_leave_dx_unwritten(pkg, T16):
    lib = _lib(pkg, T16)
    B, H, W, C, Cout, Cout2 = 2, 8, 8, 64, 128, 128
    mk = lambda *shape: torch.zeros(shape, dtype=T16, device="cuda")
    dy, wk, dy2, wk2 = mk(B * 16, Cout), mk(Cout, 9 * C), mk(B * 16, Cout2), mk(Cout2, C)
    dx = torch.full((B * H * W + 8, C), 7.0, dtype=T16, device="cuda")
    z, vec, part = mk(B * H * W, C), torch.zeros(C, device="cuda"), torch.zeros((2, C, 4), device="cuda")

    def bn(**missing):
        f = pkg._lib.MhConvBnBwd()
        f.z, f.mean, f.rstd, f.gamma, f.beta, f.part, f.relu = z.data_ptr(), vec.data_ptr(), vec.data_ptr(), vec.data_ptr(), vec.data_ptr(), part.data_ptr(), 1
        for k in missing:
            setattr(f, k, None)
        return f

    def call(dy=dy.data_ptr(), wk=wk.data_ptr(), dy2=dy2.data_ptr(), wk2=wk2.data_ptr(), ldk2=C, cout2=Cout2, dxp=dx.data_ptr(),
             geom=(B, H, W, C, 3, 2, 1, Cout, 9 * C), f=None):
        return lib.mh_conv_dgrad_pair(dy, wk, dy2, wk2, ldk2, cout2, dxp, _geom(pkg, *geom), f, _st())

    cases = {
        "odd H": (call(geom=(B, 7, 8, C, 3, 2, 1, Cout, 9 * C)), MH_ESHAPE),
        "odd W": (call(geom=(B, 8, 9, C, 3, 2, 1, Cout, 9 * C)), MH_ESHAPE),
        "Cout2 % 64": (call(cout2=96), MH_ESHAPE),
        "Cout2 = 0": (call(cout2=0), MH_ESHAPE),
        "Cout % 64": (call(geom=(B, H, W, C, 3, 2, 1, 96, 9 * C)), MH_ESHAPE),
        "ldk2 < C": (call(ldk2=0), MH_ESHAPE),
        "stride 1": (call(geom=(B, H, W, C, 3, 1, 1, Cout, 9 * C)), MH_ESHAPE),
        "a 1x1 as the first convolution": (call(geom=(B, H, W, C, 1, 2, 0, Cout, C)), MH_ESHAPE),
        "pad 0: a 3 x 3 output grid, no class on the 4 x 4 grid of the 1x1": (call(geom=(B, H, W, C, 3, 2, 0, Cout, 9 * C)), MH_ESHAPE),
        "pad 2: a 5 x 5 output grid": (call(geom=(B, H, W, C, 3, 2, 2, Cout, 9 * C)), MH_ESHAPE),
        "null dy": (call(dy=None), MH_EINVAL),
        "null wk": (call(wk=None), MH_EINVAL),
        "null dy2": (call(dy2=None), MH_EINVAL),
        "null wk2": (call(wk2=None), MH_EINVAL),
        "null dx": (call(dxp=None), MH_EINVAL),
        "misaligned dy2": (call(dy2=dy2.data_ptr() + 2), MH_EINVAL),
        "misaligned wk2": (call(wk2=wk2.data_ptr() + 8), MH_EINVAL),
        "misaligned dx": (call(dxp=dx.data_ptr() + 4), MH_EINVAL),
        "bn without z": (call(f=bn(z=None)), MH_EINVAL),
        "bn without rstd": (call(f=bn(rstd=None)), MH_EINVAL),
        "bn without part": (call(f=bn(part=None)), MH_EINVAL),
    }
    torch.cuda.synchronize()
    for what, (got, want) in cases.items():
        assert got == want, f"{what}: status {got}, expected {want}"
    assert bool((dx == 7.0).all())
    assert call(f=bn()) == 0 and call() == 0          # the same arguments, complete: accepted
    torch.cuda.synchronize()
    assert bool((dx[B * H * W:] == 7.0).all()) and bool((dx[:B * H * W] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# B. the tower
# ---------------------------------------------------------------------------------------------------------------------

BARS = {"fp16": (1e-2, 5e-2), "bf16": (6e-2, 1.5e-1)}          # (ftol, gtol) of tests/test_resnet_gpu.py's tower test
TOWERS = {"1111@64": ((1, 1, 1, 1), 64), "2111@64": ((2, 1, 1, 1), 64), "1111@48": ((1, 1, 1, 1), 48)}
PAIRS_EXPECTED = {64: 3, 48: 2}          # 48 x 48: layer 4 reads a 3 x 3 tensor -- GEMM + col2im for both of its strided convolutions
NUM_CLASSES = 10


class _RoundSTE(torch.autograd.Function):
    """x -> x rounded to the 16-bit storage type (straight-through).  `gscale` > 0: the tensor is an ACTIVATION, whose gradient the tower
    stores in 16 bits as well (the gradient stream, scaled by `gscale`): the incoming gradient is rounded the same way.  0: a weight --
    its gradient is produced in f32."""

    @staticmethod
    def forward(ctx, x, dtype, gscale):
        ctx.dtype, ctx.gscale = dtype, gscale
        return x.to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        if ctx.gscale:
            g = (g * ctx.gscale).to(ctx.dtype).to(g.dtype) / ctx.gscale
        return g, None, None


def _ref_features(p, st, image, layers, training, storage):
    """basic-block ResNet over a torchvision-keyed dict, in the arithmetic of its operands (float64: the reference); `storage`: the tower's 16-bit storage points, straight-through -- forward:
    weights, convolution inputs and outputs, BatchNorm (+ residual) (+ ReLU) outputs; backward: the gradients of those activations (the
    tower's 16-bit gradient stream: every input gradient and every BatchNorm backward's dx; x 8192 in fp16, ResNet18.gscale).
    `st`: running statistics, updated in place when training."""
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
            o = q(F.relu(bn(conv(x, p[L + "conv1.weight"], stride=s, padding=1), L + "bn1")))
            o = bn(conv(o, p[L + "conv2.weight"], padding=1), L + "bn2")
            idn = x
            if (L + "downsample.0.weight") in p:
                idn = q(bn(conv(x, p[L + "downsample.0.weight"], stride=s), L + "downsample.1"))
            x = q(F.relu(o + idn))
    return x.mean(dim=(2, 3))


def _split_state(sd):
    p = {k: v.detach().cpu().to(F64) for k, v in sd.items() if "running_" not in k and "num_batches" not in k}
    st = {k: v.detach().cpu().to(F64).clone() for k, v in sd.items() if "running_" in k}
    return p, st


# The gradient bar is 1.5 x (storage-rounded reference vs plain float64) + 0.01 per tensor: ONE realisation of the rounding noise is the
# yardstick.  At B = 2 the last stage's BatchNorms see 8 rows (2 x 2 pixels) and a single ReLU-mask flip moves a layer-4 weight gradient
# by ~sqrt(1 / 512) = 4 %, so for some inputs that yardstick does not even measure the reference itself: evaluated in float32 instead of
# float64 (same storage points, nothing of the tower involved) the reference then misses its own bar.  The seed is therefore picked on the
# CPU, from the reference alone (as part A picks its seeds): the smallest seed >= 11 for which that float32 evaluation stays within
# 1.25 x deviation + 0.01 (half the bar's margin) for every tensor of every tower and both dtypes -- 11 and 12 do not, 13 does; the test
# asserts it (at the bar itself) before looking at the GPU.  The bar the tower is held to is unchanged.
SEED = 13


def _gradient_misses(grads, ref_grads, q_grads, factor=1.5):
    """[(name, deviation from float64, the storage-rounded reference's)] of the tensors outside factor x deviation + 0.01"""
    out = []
    for name, ref in ref_grads.items():
        den = float(ref.norm()) + 1e-12
        rel, sens = float((grads[name].to(F64) - ref).norm()) / den, float((q_grads[name] - ref).norm()) / den
        if rel > factor * sens + 0.01:
            out.append((name, round(rel, 4), round(sens, 4)))
    return out


@lru_cache(maxsize=None)
def _tower_reference(pkg, tower, dtype, seed=SEED):
    """the parameters (a CPU net's own initialisation), the batch and the float64 references, plain and storage-rounded, and the
    storage-rounded one evaluated in float32: computed once"""
    layers, size = TOWERS[tower]
    T16 = F16 if dtype == "fp16" else BF16
    net = pkg.ResNet18(num_classes=NUM_CLASSES, compute_dtype=dtype, layers=layers, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for n, prm in net.named_parameters():          # BatchNorm affine parameters off their 1 / 0 defaults
        if prm.dim() == 1 and not n.startswith("fc."):
            prm.data = (torch.rand(prm.shape, generator=g) + 0.5) if n.endswith("weight") else torch.randn(prm.shape, generator=g) * 0.2
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    image = torch.randn((2, 3, size, size), generator=g)
    labels = torch.tensor([3, 8])
    p, st0 = _split_state(sd)

    def run(storage, arith=F64):
        leaves = {k: v.detach().to(arith).clone().requires_grad_(True) for k, v in p.items()}
        st = {k: v.to(arith).clone() for k, v in st0.items()}
        feats = _ref_features(leaves, st, image.to(arith), layers, True, storage)
        logits = F.linear(feats, leaves["fc.weight"], leaves["fc.bias"])
        F.cross_entropy(logits, labels).backward()
        return logits.detach(), {k: v.grad for k, v in leaves.items()}, st
    return dict(sd=sd, image=image, labels=labels, plain=run(None), rounded=run(T16), rounded_f32=run(T16, F32), T16=T16)


def _count_pairs(monkeypatch, lib, rec):
    real = lib.mh_conv_dgrad_pair

    def pair(*a):
        rec["pair"] += 1
        return real(*a)
    monkeypatch.setattr(lib, "mh_conv_dgrad_pair", pair)


@pytest.mark.parametrize("pair", [True, False], ids=["pair", "nopair"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("tower", list(TOWERS))
def test_resnet18_forward_backward_matches_float64(pkg, monkeypatch, tower, dtype, pair):
    layers, size = TOWERS[tower]
    ftol, gtol = BARS[dtype]
    r = _tower_reference(pkg, tower, dtype)
    ref_logits, ref_grads, _ = r["plain"]
    q_logits, q_grads, q_st = r["rounded"]
    assert not _gradient_misses(r["rounded_f32"][1], ref_grads, q_grads), "the reference misses its own bar in float32: SEED is no usable input"
    net = pkg.ResNet18(num_classes=NUM_CLASSES, compute_dtype=dtype, layers=layers, options=pkg.TowerOptions(pair_dgrad=pair))
    net.load_state_dict(r["sd"])
    net.cuda().train()
    rec = {"pair": 0}
    _count_pairs(monkeypatch, pkg._lib.load(dtype), rec)
    logits = net(r["image"].cuda())
    pkg.CrossEntropyLoss()(logits, r["labels"].cuda()).backward()
    torch.cuda.synchronize()
    assert rec["pair"] == (PAIRS_EXPECTED[size] if pair else 0), rec
    got_logits = logits.detach().cpu().to(F64)
    err, errq = float((got_logits - ref_logits).abs().max()), float((got_logits - q_logits).abs().max())
    sens_f = float((q_logits - ref_logits).abs().max())
    tag = f"[resnet18 {tower} {dtype} pair_dgrad={int(pair)}]"
    parity_log(f"{tag} max |logit - float64| = {err:.3e} (vs the storage-rounded reference {errq:.3e}; storage rounding alone {sens_f:.3e}; "
               f"|logit| max {float(ref_logits.abs().max()):.3f})")
    assert err < ftol * max(1.0, float(ref_logits.abs().max())) and errq < 0.5 * ftol
    worst, worst_n = ("", 0.0, 0.0), ("", 0.0)
    fails = []
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
    parity_log(f"{tag} worst gradient deviation from float64 {worst[1]:.3f} ({worst[0]}; 16-bit storage alone: {worst[2]:.3f}); "
               f"worst norm deviation from the storage-rounded reference {worst_n[1]:.3f} ({worst_n[0]})")
    assert not fails, fails[:6]
    # running statistics advance as nn.BatchNorm2d's (F.batch_norm's) do
    sd = net.state_dict()
    for k, v in q_st.items():
        bar = (2e-3 if k.endswith("running_mean") else 2e-2) * max(1.0, float(v.abs().max()))
        assert float((sd[k].cpu().to(F64) - v).abs().max()) < bar, k
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked")) and int(sd["layer4.0.downsample.1.num_batches_tracked"]) == 1
    # eval mode: the running statistics; features against the float64 composition with the same statistics
    net.eval()
    with torch.no_grad():
        feats = net.features(r["image"].cuda()).cpu().to(F64)
    p, st = _split_state(sd)
    ref_e = _ref_features(p, st, r["image"].to(F64), layers, False, None)
    q_e = _ref_features(p, st, r["image"].to(F64), layers, False, r["T16"])
    e, eq = float((feats - ref_e).abs().max()), float((feats - q_e).abs().max())
    parity_log(f"{tag} eval features: max |f - float64| = {e:.3e} (vs storage-rounded {eq:.3e}; |f| max {float(ref_e.abs().max()):.3f})")
    assert feats.shape == (2, 512) and e < ftol * max(1.0, float(ref_e.abs().max())) and eq < 0.5 * ftol
    assert all(int(v) == 1 for k, v in net.state_dict().items() if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("pair", [True, False], ids=["pair", "nopair"])
def test_resnet18_gradients_accumulate_in_place_like_autograd(pkg, pair):
    torch.manual_seed(1)
    net = pkg.ResNet18(num_classes=10, compute_dtype="fp16", layers=(1, 1, 1, 1), options=pkg.TowerOptions(pair_dgrad=pair)).cuda().train()
    g = torch.Generator().manual_seed(2)
    image = torch.randn((4, 3, 64, 64), generator=g).cuda()
    labels = torch.tensor([1, 7, 3, 3]).cuda()
    ce = pkg.CrossEntropyLoss()
    ce(net(image), labels).backward()
    first = {n: p.grad.clone() for n, p in net.named_parameters()}
    ce(net(image), labels).backward()          # .grad exists now: the in-place path
    torch.cuda.synchronize()
    for n, p in net.named_parameters():
        ref = 2.0 * first[n]
        assert float((p.grad - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-12, n
    assert int(net.bn1.num_batches_tracked) == 2 and int(net.layer4[0].downsample[1].num_batches_tracked) == 2


def test_resnet18_classifier_and_fused_adam(pkg):
    torch.manual_seed(0)
    model = pkg.ResNetClassifier(num_labels=2, compute_dtype="fp16", arch="resnet18", layers=(1, 1, 1, 1)).cuda()
    assert type(model.resnet) is pkg.ResNet18
    pkg.flatten_parameters(model)
    model.train()
    g = torch.Generator().manual_seed(3)
    batch = {"pixel_values": torch.randn((8, 3, 64, 64), generator=g).cuda(), "labels": torch.tensor([0, 1, 1, 0, 1, 0, 0, 1]).cuda()}
    opt = pkg.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss, logits = model(**batch)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert logits.shape == (8, 2) and model(pixel_values=batch["pixel_values"]).shape == (8, 2)
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_kevin_model_over_resnet18(pkg):
    kv = pkg.kevin
    tc = pkg.TextConfig(vocab_size=600, hidden=128, layers=1, heads=2, intermediate=256, max_position=64)
    cc = pkg.TextConfig(vocab_size=500, hidden=128, layers=1, heads=2, intermediate=256, max_position=64)
    model = pkg.KevinMultimodalClassifier("concatenation", text=tc, image="resnet18", caption=cc, proj=128, compute_dtype="fp16", seed=1,
                                          resnet_layers=(1, 1, 1, 1)).cuda()
    n, S = 8, 16
    g = torch.Generator().manual_seed(5)
    text, cap = torch.randint(5, 600, (n, S), generator=g), torch.randint(5, 500, (n, S), generator=g)
    mask = (torch.arange(S)[None] < torch.randint(4, S + 1, (n,), generator=g)[:, None]).long()
    image = torch.randn((n, 3, 64, 64), generator=g)
    batch = [x.cuda() for x in (text * mask, image, mask, cap * mask, mask)]
    model.eval()          # (no dropout: the two evaluations below see the same function)
    with torch.no_grad():
        out = model(*batch)
        image_output = model.image_fine_tune(model.encode_towers(batch[0], batch[1], batch[2])[1])
        direct = model.image_fine_tune(model.image_model.features(batch[1]))
    assert out.shape == (n,) and bool(torch.isfinite(out).all())
    assert image_output.shape == (n, 128) and torch.equal(image_output, direct)
    # one kevin.train step over a tiny loader moves the tower's first and last convolutions
    ids = [f"id{i}" for i in range(n)]
    ds = kv.KevinMultimodalDataset(ids, [f"words {i % 3} here" for i in range(n)], [f"{i}.png" for i in range(n)], [i % 2 for i in range(n)],
                                   captions=[f"a meme of thing {i % 3}" for i in range(n)], max_seq_len=S, image_size=64, synthetic_images=True,
                                   vocab_size=600, english_vocab_size=500)
    loader = torch.utils.data.DataLoader(ds, batch_size=n, shuffle=False, collate_fn=kv.kevin_collate)
    opt = pkg.Adam(model.get_params(2e-3), max_grad_norm=1.0)
    sched = pkg.get_linear_schedule_with_warmup(opt, num_warmup_steps=0, num_training_steps=4)
    dev = torch.device("cuda")
    pipe = pkg.data.DeviceImagePipeline(image_size=64, mode="stretch", augment=False, device=dev)
    names = ("image_model.conv1.weight", "image_model.layer4.0.downsample.0.weight", "image_fine_tune.0.weight", "text_fc.0.weight")
    before = {k: v.detach().clone() for k, v in model.named_parameters() if k in names}
    loss, _ = kv.train(model, loader, pkg.SigmoidFocalLoss(), opt, sched, dev, 0, image_pipeline=pipe, log_every=0)
    torch.cuda.synchronize()
    assert np.isfinite(loss)
    after = dict(model.named_parameters())
    for k in names:
        assert bool(torch.isfinite(after[k]).all()) and not torch.equal(after[k].detach(), before[k]), k
