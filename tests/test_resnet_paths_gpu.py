"""Every ResNet conv + BatchNorm kernel path against one plain reference: float64 torch on the CPU, computed from the same
16-bit tensors the kernels read.

The reference rounds to 16 bits exactly where a kernel stores 16 bits (the conv output z, the BatchNorm output y, the dgrad
output before it is masked, the sum with `addend`); statistics and parameter gradients stay float64.  A ReLU mask is the
kernels' own definition: round16(pre-activation) > 0, or y > 0 where a stored y / y_mask is read.  The only elements left
out are those whose pre-activation lies within one 16-bit ulp (at the scale of its terms) of zero, where the f32 arithmetic
may decide either way; there the kernel's own decision (its stored masked gradient) is taken, or their dy is zeroed.

Which path each case reaches (csrc/convgemm.hip, csrc/conv.hip, resnet.py):

  case                                    kernel / host path
  ----------------------------------------------------------------------------------------------------------------------
  fwd stem7x7s2 / 1x1 / 3x3s1 / 3x3s2 /   mh_conv_fwd(bn_part): conv_gemm_kernel<FWD> epilogue partials (generic tap walk for
      1x1s2 / C2048                         the stem's 8 padded channels), ragged M -> mh_bn2d_fwd_parts (bn2d_finish_kernel
                                            + bn2d_apply_kernel), with / without residual and ReLU
  fwd splitk                              mh_conv_fwd with workspace, mh_conv_splitk(g, 0) > 1: conv_splitk_finish_kernel partials
  standalone M=70000 / 300 / 1000x2048    mh_bn2d_fwd(training=1): bn2d_stats_kernel at the bn_rpb cap of 128 rows (547 blocks,
                                            > 64 per finish lane) and at 8 / 2 rows per block
  eval                                    mh_bn2d_fwd(training=0): bn2d_eval_stats_kernel; mh_bn2d_apply (+ residual)
  avgpool                                 mh_avgpool_fwd, mh_avgpool_bwd (scale != 1)
  bn_bwd relu_y / relu_x / plain          mh_bn2d_bwd: bn2d_bwd_stats / finish / apply with the mask from y, recomputed from x,
                                            no ReLU; dres, MH_BN_ACCUM_PARAM_GRADS, scale = 1 / 8192
  dgrad_bn 1x1 / 3x3                      mh_conv_dgrad(bn): conv_gemm_kernel<DGRAD> BatchNorm epilogue (unsplit)
  dgrad_bn splitk                         mh_conv_splitk(g, 1) > 1: conv_splitk_finish_kernel's BnFuse epilogue
  dgrad_bn strided                        3x3 / 2 on an even image: four parity-class problems, nblk = 4 ceil(B H/2 W/2 / 128)
      each with addend / y_mask NULL or set (both = the block_out fusion), relu 0 / 1, then mh_bn2d_bwd_parts
      (bn2d_bwd_finish_kernel + bn2d_bwd_apply_kernel) with and without accumulate and scale
  wgrad                                   mh_conv_wgrad at several ksplit + mh_conv_wgrad_finish_batched (accumulate 0 / 1);
                                            mh_conv_wgrad_grouped (5 mixed problems) == the single calls bit for bit
  model switches                          ResNet50(layers=(2, 1, 1, 1)) _backward_tape under ResNet50.options (TowerOptions:
                                            bn_bwd_fuse, block_out_fuse, strided_dgrad, wgrad_group): fuse_prev,
                                            pre_part and block_out are asserted to fire, and every gradient must agree

Tolerances, in units of the storage type's epsilon EPS (2^-10 fp16, 2^-7 bf16):
  * stored 16-bit tensors: |hip - ref| <= 1 ulp of the float64 value, plus TOL_SUM x (sum of |terms|) where the value is
    itself a sum or a cancellation (conv outputs, dx);
  * sums (BatchNorm partials, mean, running statistics, dgamma, dbeta, dW): |hip - ref| <= TOL_SUM x (sum of |terms|),
    the bound of f32 accumulation over blocks of <= 128 terms;
  * save_rstd: relative error <= EPS / 2, so that the statistic moves y by less than half an ulp.  The one-pass variance
    E[z^2] - mean^2 loses precision as |mean| / std grows: asserted up to 30, the error at 100 is only recorded.
Measured worst errors go through conftest.parity_log (profiles/r05_resnet_paths_parity.txt).
"""
import math

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
GSCALE = 8192.0
BN_EPS, MOMENTUM = 1e-5, 0.1
RATIOS = (0.0, 1.0, 10.0, 30.0, 100.0, None)       # per-channel |mean| / std; None = a constant channel
RATIO_ASSERT_MAX = 30.0


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


def _eps(T16):
    return 2.0 ** -MANT[T16]


def _r16(t, T16):
    """float64 -> the 16-bit value a kernel stores -> float64"""
    return t.to(T16).to(F64)


def _ulp(ref, T16):
    """the 16-bit ulp at |ref| (subnormal spacing below the smallest normal)"""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** EMIN[T16]))
    return torch.pow(2.0, (e - 1 - MANT[T16]).to(F64))


def _cpu(t):
    return t.detach().cpu().to(F64)


def _dev(t64, T16):
    return t64.to(T16).cuda().contiguous()


def _rand(shape, g, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=g, dtype=F64) * scale + shift


def _check_stored(what, got, ref, T16, terms=None, keep=None):
    """16-bit outputs: |got - ref| <= ulp(ref) (+ TOL_SUM * terms).  Returns the worst error as a fraction of the bar."""
    got = _cpu(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
    tol = _ulp(ref, T16) + (0.0 if terms is None else TOL_SUM * terms)
    err = (got - ref).abs()
    if keep is not None:
        err, tol, ref = err[keep], tol[keep], ref[keep]
    frac = err / tol
    bad = frac > 1.0
    worst = float(frac.max()) if frac.numel() else 0.0
    if bad.any():
        i = int(frac.argmax())
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} off by more than the bar; worst {worst:.3g} x bar "
                             f"(ref {float(ref.flatten()[i]):.6g}, err {float(err.flatten()[i]):.3g}, bar {float(tol.flatten()[i]):.3g})")
    return worst


def _check_sum(what, got, ref, terms, tol=TOL_SUM):
    """sums: |got - ref| <= tol * (sum of |terms|).  Returns the worst error relative to the sum of |terms|."""
    got = _cpu(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
    err = (got - ref).abs()
    rel = err / terms.clamp_min(1e-30)
    bad = err > tol * terms + 1e-30
    worst = float(rel.max()) if rel.numel() else 0.0
    if bad.any():
        i = int(rel.argmax())
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} off; worst {worst:.3g} of sum|terms| (bar {tol:.1g}; "
                             f"ref {float(ref.flatten()[i]):.6g}, got {float(got.flatten()[i]):.6g})")
    return worst


def _nhwc(x4):
    return x4.permute(0, 2, 3, 1).reshape(-1, x4.shape[1])


def _nchw(m, B, H, W):
    return m.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _geom(pkg, B, H, W, C, k, s, p, Cout, ldk):
    g = pkg._lib.MhConvGeom()
    g.B, g.H, g.W, g.C, g.KH, g.KW, g.stride, g.pad, g.Cout, g.ldk = B, H, W, C, k, k, s, p, Cout, ldk
    return g


def _pack(pkg, lib, w64, Cp, ldk, T16):
    """w64 holds 16-bit values already: the pack is exact"""
    Cout, Cin, k, _ = w64.shape
    wd = w64.to(F32).cuda().contiguous()
    wk = torch.empty((Cout, ldk), dtype=T16, device="cuda")
    pkg._lib.check(lib.mh_conv_weight_pack(wd.data_ptr(), wk.data_ptr(), Cout, Cin, k, k, Cp, ldk, _st()), "pack")
    return wk


def _ratio_channels(C, g):
    """per channel |mean| / std from RATIOS, cycling (None = a constant channel), and a random sign for the mean"""
    ratios = [RATIOS[c % len(RATIOS)] for c in range(C)]
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).to(F64)
    return ratios, sign


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward: conv -> train-mode BatchNorm (-> + residual) (-> ReLU)
# ---------------------------------------------------------------------------------------------------------------------

def _bn_stats_ref(z):
    mu = z.mean(0)
    var = ((z - mu) ** 2).mean(0)
    return mu, var


def _check_bn_forward(tag, T16, z, y, sm, sr, rm, rv, rm0, rv0, gamma, beta, r, relu, ratios):
    """z: the 16-bit BatchNorm input (float64 [M][C]); the rest device tensors / float64 reference operands."""
    M, C = z.shape
    eps16 = _eps(T16)
    mu, var = _bn_stats_ref(z)
    sm64, sr64 = _cpu(sm), _cpu(sr)
    e_mean = _check_sum(f"{tag} save_mean", sm, mu, z.abs().mean(0))
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    rel = (sr64 - rstd).abs() / rstd
    assert torch.isfinite(sr64).all() and torch.isfinite(sm64).all(), tag
    const = torch.tensor([q is None for q in ratios])
    asserted = torch.tensor([q is not None and q <= RATIO_ASSERT_MAX for q in ratios])
    e_rstd = float(rel[asserted].max())
    assert e_rstd <= eps16 / 2, f"{tag} save_rstd: relative error {e_rstd:.3g} > EPS/2 = {eps16 / 2:.3g}"
    # running statistics: momentum form, unbiased variance
    unb = var * M / (M - 1)
    rm_ref = (1 - MOMENTUM) * rm0 + MOMENTUM * mu
    rv_ref = (1 - MOMENTUM) * rv0 + MOMENTUM * unb
    e_rm = _check_sum(f"{tag} running_mean", rm, rm_ref, (1 - MOMENTUM) * rm0.abs() + MOMENTUM * z.abs().mean(0) + 1e-30)
    rv_terms = (1 - MOMENTUM) * rv0.abs() + MOMENTUM * (z * z).mean(0) * M / (M - 1)
    keep_rv = asserted | const
    e_rv = _check_sum(f"{tag} running_var", _cpu(rv)[keep_rv], rv_ref[keep_rv], rv_terms[keep_rv])
    # y from the kernel's own statistics (checked above): isolates the apply step
    v = (z - sm64) * sr64 * gamma + beta
    if r is not None:
        v = v + r
    if relu:
        v = v.clamp_min(0.0)
    terms = ((z - sm64) * sr64 * gamma).abs() + beta.abs() + (0.0 if r is None else r.abs())
    e_y = _check_stored(f"{tag} y", y, v, T16, terms=terms)
    if const.any() and r is None:      # variance 0: mean == z exactly, so y is beta (through the ReLU) bit for bit
        want = beta[const].clamp_min(0.0) if relu else beta[const]
        assert torch.equal(_cpu(y)[:, const], _r16(want, T16).expand(M, -1)), f"{tag}: a constant channel's y must equal beta"
    errs = dict(mean=e_mean, rstd=e_rstd, run_mean=e_rm, run_var=e_rv, y=e_y)
    hi = torch.tensor([q == 100.0 for q in ratios])
    if hi.any():      # recorded, not asserted: the one-pass variance at |mean| / std = 100
        errs["rstd_r100"] = float(rel[hi].max())
        errs["run_var_r100"] = float(((_cpu(rv) - rv_ref).abs() / rv_ref)[hi].max())
    return errs


def _log(tag, errs):
    parity_log(f"[resnet {tag}] " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))


# (B, Cin, H, W, Cout, k, stride, pad, Cp): every ResNet-50 conv class at a ragged M (B*Ho*Wo not a multiple of 128)
FWD_GEOMS = {
    "stem7x7s2": (2, 3, 30, 30, 64, 7, 2, 3, 8),       # M = 450, the generic tap walk over 8 padded channels
    "1x1": (3, 64, 15, 15, 256, 1, 1, 0, 64),          # M = 675
    "3x3s1": (2, 64, 14, 13, 64, 3, 1, 1, 64),         # M = 364
    "3x3s2": (2, 64, 17, 17, 128, 3, 2, 1, 64),        # M = 162
    "1x1s2": (2, 256, 14, 14, 512, 1, 2, 0, 256),      # M = 98, the downsample
    "C2048": (2, 512, 7, 7, 2048, 1, 1, 0, 512),       # M = 98, 2048 channels
    "splitk": (2, 2048, 7, 7, 512, 1, 1, 0, 2048),     # M = 98, split-K forward (asserted)
}


def _conv_inputs(B, Cin, H, W, Cout, k, Cp, g, T16, ratios=None, sign=None):
    """x [B][Cin][H][W], w [Cout][Cin][k][k], float64 holding 16-bit values.  With `ratios` (1x1 only): input channel 0 is
    the constant 1 and output channel c gets the offset ratio * sign on it over a unit-variance remainder."""
    x = _r16(_rand((B, Cin, H, W), g), T16)
    w = _r16(_rand((Cout, Cin, k, k), g, 1.0 / math.sqrt(Cin * k * k)), T16)
    if ratios is not None:
        x[:, 0] = 1.0
        w = _r16(_rand((Cout, Cin, k, k), g, 1.0 / math.sqrt(Cin - 1)), T16)
        for c, q in enumerate(ratios):
            if q is None:
                w[c] = 0.0
                w[c, 0] = _r16(torch.tensor(2.71 * float(sign[c]), dtype=F64), T16)
            else:
                w[c, 0] = _r16(torch.tensor(q * float(sign[c]), dtype=F64), T16)
    xp = torch.zeros((B, Cp, H, W), dtype=F64)
    xp[:, :Cin] = x
    return x, w, xp


@DTYPES
@pytest.mark.parametrize("case", list(FWD_GEOMS))
def test_conv_bn_forward(pkg, case, T16):
    lib = _lib(pkg, T16)
    B, Cin, H, W, Cout, k, s, p, Cp = FWD_GEOMS[case]
    g = torch.Generator().manual_seed(100 + len(case) * 7 + Cout)
    use_ratios = k == 1
    ratios, sign = _ratio_channels(Cout, g) if use_ratios else ([0.0] * Cout, None)
    x, w, xp = _conv_inputs(B, Cin, H, W, Cout, k, Cp, g, T16, ratios if use_ratios else None, sign)
    ref = F.conv2d(x, w, stride=s, padding=p)
    terms = F.conv2d(x.abs(), w.abs(), stride=s, padding=p)
    Ho, Wo = ref.shape[2], ref.shape[3]
    M = B * Ho * Wo
    assert M % 128, case
    ldk = (k * k * Cp + 63) // 64 * 64
    geom = _geom(pkg, B, H, W, Cp, k, s, p, Cout, ldk)
    sp = int(lib.mh_conv_splitk(geom, 0))
    assert (sp > 1) == (case == "splitk"), (case, sp)          # every other case runs the unsplit epilogue
    ws = torch.empty((sp, M, Cout), dtype=F32, device="cuda") if sp > 1 else None
    xd, wk = _dev(_nhwc(xp), T16), _pack(pkg, lib, w, Cp, ldk, T16)
    nblk = (M + 127) // 128
    z = torch.full((M, Cout), 7.0, dtype=T16, device="cuda")
    part = torch.full((2, Cout, nblk), float("nan"), dtype=F32, device="cuda")
    pkg._lib.check(lib.mh_conv_fwd(xd.data_ptr(), wk.data_ptr(), z.data_ptr(), part.data_ptr(), None if ws is None else ws.data_ptr(),
                                   geom, _st()), "mh_conv_fwd")
    torch.cuda.synchronize()
    e_z = _check_stored(f"{case} {_name(T16)} z", z, _nhwc(ref), T16, terms=_nhwc(terms))
    # per-128-row-tile partials of the stored values; rows past M count nothing
    z64 = _cpu(z)
    tile = torch.arange(M) // 128
    s0 = torch.zeros((nblk, Cout), dtype=F64).index_add_(0, tile, z64)
    s1 = torch.zeros((nblk, Cout), dtype=F64).index_add_(0, tile, z64 * z64)
    a0 = torch.zeros((nblk, Cout), dtype=F64).index_add_(0, tile, z64.abs())
    e_p0 = _check_sum(f"{case} part sum z", part[0], s0.t(), a0.t())
    e_p1 = _check_sum(f"{case} part sum z^2", part[1], s1.t(), s1.t())
    parity_log(f"[resnet fwd {case} {_name(T16)}] z {e_z:.3e} xbar, part {max(e_p0, e_p1):.3e} of sum|terms| (M {M}, split {sp})")
    # the model's BatchNorm: mh_bn2d_fwd_parts with and without residual / ReLU
    gamma = torch.rand(Cout, generator=g, dtype=F64) + 0.5
    beta = _rand(Cout, g, 0.3)
    gd, bd = gamma.to(F32).cuda(), beta.to(F32).cuda()
    gamma, beta = gamma.to(F32).to(F64), beta.to(F32).to(F64)
    for (res, relu) in ((False, True), (True, True), (False, False)):
        r = _r16(_rand((M, Cout), g), T16) if res else None
        rd = _dev(r, T16) if res else None
        rm0 = _rand(Cout, g, 0.2).to(F32).to(F64)
        rv0 = (torch.rand(Cout, generator=g, dtype=F64) + 0.5).to(F32).to(F64)
        rm, rv = rm0.to(F32).cuda(), rv0.to(F32).cuda()
        y = torch.full((M, Cout), 7.0, dtype=T16, device="cuda")
        sm, sr = torch.full((Cout,), float("nan"), device="cuda"), torch.full((Cout,), float("nan"), device="cuda")
        pkg._lib.check(lib.mh_bn2d_fwd_parts(z.data_ptr(), part.data_ptr(), nblk, gd.data_ptr(), bd.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                             None if rd is None else rd.data_ptr(), y.data_ptr(), sm.data_ptr(), sr.data_ptr(), M, Cout,
                                             BN_EPS, MOMENTUM, int(relu), _st()), "mh_bn2d_fwd_parts")
        torch.cuda.synchronize()
        tag = f"fwd {case} {_name(T16)} res={int(res)} relu={int(relu)}"
        _log(tag, _check_bn_forward(tag, T16, z64, y, sm, sr, rm, rv, rm0, rv0, gamma, beta, r, relu, ratios))


# (M, C): the bn_rpb cap (128 rows per block, 547 blocks: > 64 per finish lane), M < 512 (8 rows per block), 2048 channels
STANDALONE = {"M70000": (70000, 64), "M300": (300, 256), "M1000xC2048": (1000, 2048)}


@DTYPES
@pytest.mark.parametrize("case", list(STANDALONE))
def test_bn_forward_standalone(pkg, case, T16):
    lib = _lib(pkg, T16)
    M, C = STANDALONE[case]
    g = torch.Generator().manual_seed(200 + M + C)
    ratios, sign = _ratio_channels(C, g)
    std = torch.rand(C, generator=g, dtype=F64) * 1.5 + 0.5
    off = torch.tensor([0.0 if q is None else q for q in ratios], dtype=F64) * sign * std
    x = _rand((M, C), g) * std + off
    for c, q in enumerate(ratios):
        if q is None:
            x[:, c] = 2.71 * float(sign[c])
    x = _r16(x, T16)
    xd = _dev(x, T16)
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).to(F32).to(F64)
    beta = _rand(C, g, 0.3).to(F32).to(F64)
    gd, bd = gamma.to(F32).cuda(), beta.to(F32).cuda()
    ws = torch.empty(int(lib.mh_bn2d_workspace_elems(M, C)), dtype=F32, device="cuda")
    for (res, relu) in ((False, True), (True, True), (False, False)):
        r = _r16(_rand((M, C), g), T16) if res else None
        rd = _dev(r, T16) if res else None
        rm0 = _rand(C, g, 0.2).to(F32).to(F64)
        rv0 = (torch.rand(C, generator=g, dtype=F64) + 0.5).to(F32).to(F64)
        rm, rv = rm0.to(F32).cuda(), rv0.to(F32).cuda()
        y = torch.full((M, C), 7.0, dtype=T16, device="cuda")
        sm, sr = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
        pkg._lib.check(lib.mh_bn2d_fwd(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                       None if rd is None else rd.data_ptr(), y.data_ptr(), sm.data_ptr(), sr.data_ptr(), ws.data_ptr(),
                                       M, C, BN_EPS, MOMENTUM, 1, int(relu), _st()), "mh_bn2d_fwd")
        torch.cuda.synchronize()
        tag = f"bn_fwd {case} {_name(T16)} res={int(res)} relu={int(relu)}"
        _log(tag, _check_bn_forward(tag, T16, x, y, sm, sr, rm, rv, rm0, rv0, gamma, beta, r, relu, ratios))


# ---------------------------------------------------------------------------------------------------------------------
# 2. eval mode and pools
# ---------------------------------------------------------------------------------------------------------------------

@DTYPES
def test_bn_eval_mode_and_apply(pkg, T16):
    lib = _lib(pkg, T16)
    g = torch.Generator().manual_seed(300)
    M, C = 777, 96
    x = _r16(_rand((M, C), g, 1.3, 0.4), T16)
    xd = _dev(x, T16)
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).to(F32).to(F64)
    beta = _rand(C, g, 0.3).to(F32).to(F64)
    gd, bd = gamma.to(F32).cuda(), beta.to(F32).cuda()
    rm0 = _rand(C, g, 0.5).to(F32)
    rv0 = torch.exp(torch.empty(C, dtype=F64).uniform_(math.log(1e-4), math.log(10.0), generator=g)).to(F32)   # eps matters at 1e-4
    errs = {}
    for (res, relu) in ((False, True), (True, True), (False, False)):
        r = _r16(_rand((M, C), g), T16) if res else None
        rd = _dev(r, T16) if res else None
        rm, rv = rm0.cuda(), rv0.cuda()
        y = torch.full((M, C), 7.0, dtype=T16, device="cuda")
        sm, sr = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
        pkg._lib.check(lib.mh_bn2d_fwd(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                       None if rd is None else rd.data_ptr(), y.data_ptr(), sm.data_ptr(), sr.data_ptr(), None,
                                       M, C, BN_EPS, MOMENTUM, 0, int(relu), _st()), "mh_bn2d_fwd eval")
        torch.cuda.synchronize()
        assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0), "eval mode must not touch the running statistics"
        assert torch.equal(sm.cpu(), rm0), "eval mode normalises with the running mean"
        rstd = 1.0 / torch.sqrt(rv0.to(F64) + BN_EPS)
        e_r = float(((_cpu(sr) - rstd).abs() / rstd).max())
        assert e_r <= 4 * 2.0 ** -24, f"eval rstd: relative error {e_r:.3g}"
        v = (x - rm0.to(F64)) * rstd * gamma + beta + (0.0 if r is None else r)
        v = v.clamp_min(0.0) if relu else v
        terms = ((x - rm0.to(F64)) * rstd * gamma).abs() + beta.abs() + (0.0 if r is None else r.abs())
        e_y = _check_stored(f"eval res={int(res)} relu={int(relu)} y", y, v, T16, terms=terms)
        # mh_bn2d_apply with arbitrary statistics
        mean_a = _rand(C, g, 0.5).to(F32)
        rstd_a = (torch.rand(C, generator=g, dtype=F64) * 2 + 0.2).to(F32)
        ya = torch.full((M, C), 7.0, dtype=T16, device="cuda")
        md, rsd = mean_a.cuda(), rstd_a.cuda()
        pkg._lib.check(lib.mh_bn2d_apply(xd.data_ptr(), md.data_ptr(), rsd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                         None if rd is None else rd.data_ptr(), ya.data_ptr(), M, C, int(relu), _st()), "mh_bn2d_apply")
        torch.cuda.synchronize()
        xh = (x - mean_a.to(F64)) * rstd_a.to(F64)
        va = xh * gamma + beta + (0.0 if r is None else r)
        va = va.clamp_min(0.0) if relu else va
        ta = (xh * gamma).abs() + beta.abs() + (0.0 if r is None else r.abs())
        e_a = _check_stored(f"apply res={int(res)} relu={int(relu)} y", ya, va, T16, terms=ta)
        errs[f"res={int(res)},relu={int(relu)}"] = max(e_y, e_a)
    _log(f"eval+apply {_name(T16)}", dict(rstd=e_r, **{f"y[{k}]": v for k, v in errs.items()}))


@DTYPES
def test_avgpool_forward_and_backward(pkg, T16):
    lib = _lib(pkg, T16)
    g = torch.Generator().manual_seed(301)
    errs = {}
    for (B, HW, C) in ((3, 49, 2048), (2, 4, 264), (1, 1, 16)):
        x = _r16(_rand((B * HW, C), g, 1.0, 0.5), T16)
        y = torch.full((B, C), float("nan"), device="cuda")
        pkg._lib.check(lib.mh_avgpool_fwd(_dev(x, T16).data_ptr(), y.data_ptr(), B, HW, C, _st()), "mh_avgpool_fwd")
        xv = x.view(B, HW, C)
        dy = _rand((B, C), g).to(F32)
        dx = torch.full((B * HW, C), 7.0, dtype=T16, device="cuda")
        pkg._lib.check(lib.mh_avgpool_bwd(dy.cuda().data_ptr(), dx.data_ptr(), B, HW, C, GSCALE, _st()), "mh_avgpool_bwd")
        torch.cuda.synchronize()
        e_f = _check_sum(f"avgpool fwd {B}x{HW}x{C}", y, xv.mean(1), xv.abs().mean(1))
        want = (dy.to(F64) * GSCALE / HW)[:, None, :].expand(B, HW, C).reshape(B * HW, C)
        e_b = _check_stored(f"avgpool bwd {B}x{HW}x{C}", dx, want, T16)
        errs[f"{B}x{HW}x{C}"] = max(e_f, e_b)
    _log(f"avgpool {_name(T16)}", errs)


# ---------------------------------------------------------------------------------------------------------------------
# 3. BatchNorm backward, every variant
# ---------------------------------------------------------------------------------------------------------------------

def _batch_stats(z):
    """batch mean / rstd of z (float64 [M][C]) as the f32 a forward would have saved, and float64"""
    mu, var = _bn_stats_ref(z)
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    return mu.to(F32), rstd.to(F32)


def _bn_bwd_ref(z, gamma, gp, scale):
    """float64 autograd of bn(z) (train mode, batch statistics) with the (masked) incoming gradient gp"""
    zr = z.clone().requires_grad_(True)
    ga = gamma.clone().requires_grad_(True)
    be = torch.zeros_like(gamma, requires_grad=True)
    mu = zr.mean(0)
    var = ((zr - mu) ** 2).mean(0)
    out = (zr - mu) / torch.sqrt(var + BN_EPS) * ga + be
    out.backward(gp)
    return zr.grad, ga.grad * scale, be.grad * scale


def _check_bn_bwd(tag, T16, z, mean, rstd, gamma, gp, dx, dg, db, scale, dg0=None, db0=None):
    M = z.shape[0]
    xh = (z - mean.to(F64)) * rstd.to(F64)
    dx_ref, dg_ref, db_ref = _bn_bwd_ref(z, gamma, gp, scale)
    s_abs, q_abs = gp.abs().sum(0), (gp * xh).abs().sum(0)
    terms = gamma.abs() * rstd.to(F64) * (gp.abs() + s_abs / M + xh.abs() * q_abs / M)
    e_dx = _check_stored(f"{tag} dx", dx, dx_ref, T16, terms=terms)
    if dg0 is not None:
        dg_ref, db_ref = dg_ref + dg0, db_ref + db0
    e_dg = _check_sum(f"{tag} dgamma", dg, dg_ref, scale * q_abs + (0.0 if dg0 is None else dg0.abs()))
    e_db = _check_sum(f"{tag} dbeta", db, db_ref, scale * s_abs + (0.0 if db0 is None else db0.abs()))
    return dict(dx=e_dx, dgamma=e_dg, dbeta=e_db)


BN_BWD_VARIANTS = ["relu_y", "relu_x", "plain"]


@DTYPES
@pytest.mark.parametrize("variant", BN_BWD_VARIANTS)
@pytest.mark.parametrize("M,C", [(900, 64), (70000, 64), (300, 2048)], ids=["M900", "M70000", "M300xC2048"])
def test_bn2d_backward(pkg, M, C, variant, T16):
    lib = _lib(pkg, T16)
    g = torch.Generator().manual_seed(400 + M + C + BN_BWD_VARIANTS.index(variant))
    z = _r16(_rand((M, C), g, 1.3, 0.2), T16)
    mean, rstd = _batch_stats(z)
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).to(F32).to(F64)
    beta = _rand(C, g, 0.5).to(F32).to(F64)
    xh = (z - mean.to(F64)) * rstd.to(F64)
    dy = _r16((_rand((M, C), g) + xh) * 64.0, T16)         # correlated with xhat: sum dy' xhat is not small
    relu = variant != "plain"
    y = None
    if variant == "relu_y":        # y = relu(bn(z) + residual): the mask is y > 0 of the stored output
        r = _r16(_rand((M, C), g), T16)
        y = _r16((xh * gamma + beta + r).clamp_min(0.0), T16)
        keep = y > 0
    elif variant == "relu_x":      # mask recomputed from z: round16(xhat gamma + beta) > 0; dy = 0 where that is a rounding call
        v = xh * gamma + beta
        unsure = v.abs() <= _ulp((xh * gamma).abs() + beta.abs(), T16)
        dy[unsure] = 0.0
        keep = _r16(v, T16) > 0
    else:
        keep = torch.ones_like(z, dtype=torch.bool)
    gp = torch.where(keep, dy, torch.zeros_like(dy))
    zd, dyd = _dev(z, T16), _dev(dy, T16)
    yd = _dev(y, T16) if y is not None else None
    md, rsd, gd, bd = mean.cuda(), rstd.cuda(), gamma.to(F32).cuda(), beta.to(F32).cuda()
    ws = torch.empty(int(lib.mh_bn2d_workspace_elems(M, C)), dtype=F32, device="cuda")
    errs = {}
    for (want_dres, accum, scale) in ((False, False, 1.0), (True, True, 1.0 / GSCALE)):
        dx = torch.full((M, C), 7.0, dtype=T16, device="cuda")
        dres = torch.full((M, C), 7.0, dtype=T16, device="cuda") if want_dres else None
        dg0 = _rand(C, g).to(F32) if accum else None
        db0 = _rand(C, g).to(F32) if accum else None
        dg = dg0.cuda() if accum else torch.full((C,), float("nan"), device="cuda")
        db = db0.cuda() if accum else torch.full((C,), float("nan"), device="cuda")
        flags = (pkg._lib.MH_BN_RELU if relu else 0) | (pkg._lib.MH_BN_ACCUM_PARAM_GRADS if accum else 0)
        pkg._lib.check(lib.mh_bn2d_bwd(dyd.data_ptr(), zd.data_ptr(), None if yd is None else yd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                       md.data_ptr(), rsd.data_ptr(), dx.data_ptr(), None if dres is None else dres.data_ptr(),
                                       dg.data_ptr(), db.data_ptr(), ws.data_ptr(), M, C, flags, scale, _st()), "mh_bn2d_bwd")
        torch.cuda.synchronize()
        tag = f"bn_bwd {variant} M={M} C={C} {_name(T16)} dres={int(want_dres)} accum={int(accum)} scale={scale:g}"
        e = _check_bn_bwd(tag, T16, z, mean, rstd, gamma, gp, dx, dg, db, scale,
                          None if dg0 is None else dg0.to(F64), None if db0 is None else db0.to(F64))
        if want_dres:
            e["dres"] = _check_stored(f"{tag} dres", dres, gp, T16)
        errs.update({f"{k}{'[acc]' if accum else ''}": v for k, v in e.items()})
    _log(f"bn_bwd {variant} M={M} C={C} {_name(T16)}", errs)


# (B, C, H, W, Cout, k, stride, pad): the convolution whose INPUT gradient feeds the BatchNorm backward (C channels)
DGRAD_GEOMS = {
    "1x1": (2, 256, 15, 15, 64, 1, 1, 0),        # a block's conv1: the block_out fusion's shape; M = 450
    "3x3": (2, 64, 14, 13, 64, 3, 1, 1),         # unsplit; M = 364
    "splitk": (2, 512, 7, 7, 512, 3, 1, 1),      # mh_conv_splitk(g, 1) > 1: the split-K finish epilogue; M = 98
    "strided": (2, 64, 18, 18, 128, 3, 2, 1),    # parity classes: 4 x 2 tiles of 162 rows each
}
FUSE_SETTINGS = [(add, ym, relu) for add in (False, True) for ym in (False, True) for relu in (1, 0)]


def _dgrad_tiles(B, H, W, s):
    """the partial column (tile) of every input-gradient row: 128-row tiles, per parity class for the strided launch"""
    if s == 1:
        return torch.arange(B * H * W) // 128, (B * H * W + 127) // 128
    Hh, Wh = H // 2, W // 2
    per = (B * Hh * Wh + 127) // 128
    b = torch.arange(B)[:, None, None]
    h = torch.arange(H)[None, :, None]
    w = torch.arange(W)[None, None, :]
    cls = (h % 2) * 2 + (w % 2)
    r = (b * Hh + h // 2) * Wh + w // 2
    return (cls * per + r // 128).reshape(-1), 4 * per


@DTYPES
@pytest.mark.parametrize("case", list(DGRAD_GEOMS))
def test_dgrad_bn_epilogue_and_bwd_parts(pkg, case, T16):
    lib = _lib(pkg, T16)
    B, C, H, W, Cout, k, s, p = DGRAD_GEOMS[case]
    g = torch.Generator().manual_seed(500 + Cout + C + s)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    Mi = B * H * W
    ldk = k * k * C
    geom = _geom(pkg, B, H, W, C, k, s, p, Cout, ldk)
    sp = int(lib.mh_conv_splitk(geom, 1))
    assert (sp > 1) == (case == "splitk"), (case, sp)
    ws = torch.empty((sp, Mi, C), dtype=F32, device="cuda") if sp > 1 else None
    wsp = None if ws is None else ws.data_ptr()
    w = _r16(_rand((Cout, C, k, k), g, 1.0 / math.sqrt(Cout * k * k / s / s)), T16)
    dy = _r16(_rand((B, Cout, Ho, Wo), g), T16)
    wk, dyd = _pack(pkg, lib, w, C, ldk, T16), _dev(_nhwc(dy), T16)
    # the plain input gradient: the dy of the BatchNorm below, as stored
    dx_plain = torch.full((Mi, C), 7.0, dtype=T16, device="cuda")
    pkg._lib.check(lib.mh_conv_dgrad(dyd.data_ptr(), wk.data_ptr(), dx_plain.data_ptr(), wsp, geom, None, _st()), "mh_conv_dgrad")
    torch.cuda.synchronize()
    xr = torch.zeros((B, C, H, W), dtype=F64, requires_grad=True)
    F.conv2d(xr, w, stride=s, padding=p).backward(dy)
    xa = torch.zeros((B, C, H, W), dtype=F64, requires_grad=True)
    F.conv2d(xa, w.abs(), stride=s, padding=p).backward(dy.abs())
    e_d = _check_stored(f"dgrad {case} {_name(T16)}", dx_plain, _nhwc(xr.grad), T16, terms=_nhwc(xa.grad))
    D = _cpu(dx_plain)
    # the BatchNorm whose output is this convolution's input
    z = _r16(_rand((Mi, C), g, 1.3, 0.2), T16)
    mean, rstd = _batch_stats(z)
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).to(F32).to(F64)
    beta = _rand(C, g, 0.5).to(F32).to(F64)
    xh = (z - mean.to(F64)) * rstd.to(F64)
    v = xh * gamma + beta
    res = _r16(_rand((Mi, C), g), T16)
    y_mask = _r16((v + res).clamp_min(0.0), T16)           # the block's stored output relu(bn3(z) + residual)
    addend = _r16(_rand((Mi, C), g), T16)
    zd, md, rsd, gd, bd = _dev(z, T16), mean.cuda(), rstd.cuda(), gamma.to(F32).cuda(), beta.to(F32).cuda()
    ymd, add_d = _dev(y_mask, T16), _dev(addend, T16)
    tiles, nblk = _dgrad_tiles(B, H, W, s)
    if s == 2:
        assert nblk == 4 * ((B * (H // 2) * (W // 2) + 127) // 128)
    unsure_z = v.abs() <= _ulp((xh * gamma).abs() + beta.abs(), T16)
    for (add, ym, relu) in FUSE_SETTINGS:
        tag = f"dgrad_bn {case} {_name(T16)} addend={int(add)} y_mask={int(ym)} relu={relu}"
        f = pkg._lib.MhConvBnBwd()
        part = torch.full((2, C, nblk), float("nan"), dtype=F32, device="cuda")
        f.z, f.mean, f.rstd, f.gamma, f.beta, f.part, f.relu = zd.data_ptr(), md.data_ptr(), rsd.data_ptr(), gd.data_ptr(), bd.data_ptr(), part.data_ptr(), relu
        f.addend = add_d.data_ptr() if add else None
        f.y_mask = ymd.data_ptr() if ym else None
        gm = torch.full((Mi, C), 7.0, dtype=T16, device="cuda")
        pkg._lib.check(lib.mh_conv_dgrad(dyd.data_ptr(), wk.data_ptr(), gm.data_ptr(), wsp, geom, f, _st()), "mh_conv_dgrad(bn)")
        torch.cuda.synchronize()
        gsum = _r16(D + addend, T16) if add else D           # mh_add_h16's rounding of the sum
        if not relu:
            keep, unsure = torch.ones_like(z, dtype=torch.bool), torch.zeros_like(z, dtype=torch.bool)
        elif ym:
            keep, unsure = y_mask > 0, torch.zeros_like(z, dtype=torch.bool)
        else:
            keep, unsure = _r16(v, T16) > 0, unsure_z
        got = _cpu(gm)
        gp = torch.where(keep, gsum, torch.zeros_like(gsum))
        gp = torch.where(unsure, got, gp)                     # a rounding call either way: the kernel's decision
        e_g = _check_stored(f"{tag} masked gradient", gm, gp, T16)
        s0 = torch.zeros((nblk, C), dtype=F64).index_add_(0, tiles, gp)
        s1 = torch.zeros((nblk, C), dtype=F64).index_add_(0, tiles, gp * xh)
        a0 = torch.zeros((nblk, C), dtype=F64).index_add_(0, tiles, gp.abs())
        a1 = torch.zeros((nblk, C), dtype=F64).index_add_(0, tiles, (gp * xh).abs())
        e_p = max(_check_sum(f"{tag} part sum g'", part[0], s0.t(), a0.t()),
                  _check_sum(f"{tag} part sum g' xhat", part[1], s1.t(), a1.t()))
        errs = dict(dgrad=e_d, masked=e_g, part=e_p)
        for (accum, scale) in ((False, 1.0), (True, 1.0 / GSCALE)):
            dx = torch.full((Mi, C), 7.0, dtype=T16, device="cuda")
            dg0, db0 = (_rand(C, g).to(F32), _rand(C, g).to(F32)) if accum else (None, None)
            dg = dg0.cuda() if accum else torch.full((C,), float("nan"), device="cuda")
            db = db0.cuda() if accum else torch.full((C,), float("nan"), device="cuda")
            sums = torch.full((2, C), float("nan"), device="cuda")
            pkg._lib.check(lib.mh_bn2d_bwd_parts(gm.data_ptr(), zd.data_ptr(), part.data_ptr(), nblk, gd.data_ptr(), md.data_ptr(), rsd.data_ptr(),
                                                 dx.data_ptr(), dg.data_ptr(), db.data_ptr(), sums.data_ptr(), Mi, C,
                                                 pkg._lib.MH_BN_ACCUM_PARAM_GRADS if accum else 0, scale, _st()), "mh_bn2d_bwd_parts")
            torch.cuda.synchronize()
            e = _check_bn_bwd(f"{tag} accum={int(accum)}", T16, z, mean, rstd, gamma, gp, dx, dg, db, scale,
                              None if dg0 is None else dg0.to(F64), None if db0 is None else db0.to(F64))
            errs.update({f"{k}{'[acc]' if accum else ''}": v for k, v in e.items()})
        _log(tag, errs)


# ---------------------------------------------------------------------------------------------------------------------
# 4. weight gradients
# ---------------------------------------------------------------------------------------------------------------------

# (B, Cin, H, W, Cout, k, stride, pad, Cp)
WGRAD_GEOMS = [
    (2, 3, 30, 30, 64, 7, 2, 3, 8),        # stem: 3 channels padded to 8, ldk 448 > 392
    (3, 64, 15, 15, 256, 1, 1, 0, 64),
    (2, 64, 14, 13, 64, 3, 1, 1, 64),
    (2, 128, 17, 17, 128, 3, 2, 1, 128),
    (2, 256, 14, 14, 512, 1, 2, 0, 256),
]


def _wgrad_problem(pkg, lib, T16, geo, g):
    B, Cin, H, W, Cout, k, s, p, Cp = geo
    x = _r16(_rand((B, Cin, H, W), g), T16)
    xp = torch.zeros((B, Cp, H, W), dtype=F64)
    xp[:, :Cin] = x
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = _r16(_rand((B, Cout, Ho, Wo), g), T16)
    ldk = (k * k * Cp + 63) // 64 * 64
    wr = torch.zeros((Cout, Cin, k, k), dtype=F64, requires_grad=True)
    F.conv2d(x, wr, stride=s, padding=p).backward(dy)
    wa = torch.zeros((Cout, Cin, k, k), dtype=F64, requires_grad=True)
    F.conv2d(x.abs(), wa, stride=s, padding=p).backward(dy.abs())
    return dict(xd=_dev(_nhwc(xp), T16), dyd=_dev(_nhwc(dy), T16), geom=_geom(pkg, B, H, W, Cp, k, s, p, Cout, ldk), M=B * Ho * Wo,
                ldk=ldk, Cout=Cout, Cin=Cin, k=k, Cp=Cp, ref=wr.grad, terms=wa.grad)


def _finish(pkg, lib, jobs_in, accumulate):
    """mh_conv_wgrad_finish_batched over [(problem, slabs, sp, scale, g)] in one launch"""
    jobs = (pkg._lib.MhConvWgradJob * len(jobs_in))()
    for j, (pr, slabs, sp, scale, gt) in enumerate(jobs_in):
        jobs[j].slabs, jobs[j].g = slabs.data_ptr(), gt.data_ptr()
        jobs[j].Cout, jobs[j].Cin, jobs[j].KH, jobs[j].KW, jobs[j].Cp, jobs[j].ldk = pr["Cout"], pr["Cin"], pr["k"], pr["k"], pr["Cp"], pr["ldk"]
        jobs[j].nsplit, jobs[j].accumulate, jobs[j].scale = sp, int(accumulate), scale
    pkg._lib.check(lib.mh_conv_wgrad_finish_batched(jobs, len(jobs_in), _st()), "mh_conv_wgrad_finish_batched")


@DTYPES
def test_conv_wgrad_ksplit_and_finish(pkg, T16):
    lib = _lib(pkg, T16)
    g = torch.Generator().manual_seed(600)
    errs = {}
    for gi, geo in enumerate(WGRAD_GEOMS):
        pr = _wgrad_problem(pkg, lib, T16, geo, g)
        splits = sorted({max(1, int(lib.mh_gemm_ksplit_for(pr["M"], want))) for want in (1, 3, 8)})
        assert len(splits) > 1, (geo, splits)
        for sp in splits:
            for accum in (False, True):
                alpha, scale = (1.0 / GSCALE, 2.0) if accum else (1.0, 1.0)
                slabs = torch.full((sp, pr["Cout"], pr["ldk"]), 5.0, dtype=F32, device="cuda")
                pkg._lib.check(lib.mh_conv_wgrad(pr["dyd"].data_ptr(), pr["xd"].data_ptr(), slabs.data_ptr(), sp, alpha, pr["geom"], _st()),
                               "mh_conv_wgrad")
                g0 = _rand(pr["ref"].shape, g).to(F32)
                gt = g0.cuda() if accum else torch.full(pr["ref"].shape, float("nan"), device="cuda")
                _finish(pkg, lib, [(pr, slabs, sp, scale, gt)], accum)
                torch.cuda.synchronize()
                want = alpha * scale * pr["ref"] + (g0.to(F64) if accum else 0.0)
                terms = abs(alpha * scale) * pr["terms"] + (g0.to(F64).abs() if accum else 0.0)
                e = _check_sum(f"wgrad {geo} split {sp} accumulate {int(accum)} {_name(T16)}", gt, want, terms)
                errs[f"g{gi}/sp{sp}{'/acc' if accum else ''}"] = e
    _log(f"wgrad {_name(T16)}", {"worst": max(errs.values())})
    parity_log("    " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))


@DTYPES
@pytest.mark.parametrize("n", [2, 5])
def test_conv_wgrad_grouped_equals_single_calls(pkg, n, T16):
    lib = _lib(pkg, T16)
    g = torch.Generator().manual_seed(700 + n)
    geos = WGRAD_GEOMS[:n] if n == 5 else [WGRAD_GEOMS[3], WGRAD_GEOMS[0]]
    prs = [_wgrad_problem(pkg, lib, T16, geo, g) for geo in geos]
    probs = (pkg._lib.MhConvWgradProblem * n)()
    singles, groups = [], []
    for i, pr in enumerate(prs):
        sp = max(1, int(lib.mh_gemm_ksplit_for(pr["M"], 2 + i)))
        one = torch.full((sp, pr["Cout"], pr["ldk"]), 5.0, dtype=F32, device="cuda")
        pkg._lib.check(lib.mh_conv_wgrad(pr["dyd"].data_ptr(), pr["xd"].data_ptr(), one.data_ptr(), sp, 1.0 / GSCALE, pr["geom"], _st()),
                       "mh_conv_wgrad")
        grp = torch.full_like(one, -5.0)
        probs[i].dy, probs[i].x, probs[i].slabs = pr["dyd"].data_ptr(), pr["xd"].data_ptr(), grp.data_ptr()
        probs[i].ksplit, probs[i].alpha, probs[i].geom = sp, 1.0 / GSCALE, pr["geom"]
        singles.append((pr, one, sp))
        groups.append((pr, grp, sp))
    pkg._lib.check(lib.mh_conv_wgrad_grouped(probs, n, _st()), "mh_conv_wgrad_grouped")
    torch.cuda.synchronize()
    for (pr, one, sp), (_, grp, _) in zip(singles, groups):
        kc = pr["k"] * pr["k"] * pr["Cp"]          # (the columns past KH*KW*Cp of the ldk pitch are never written)
        assert torch.equal(one[:, :, :kc], grp[:, :, :kc]), f"grouped slabs differ from the single call ({pr['geom'].KH}x{pr['geom'].KW}/{pr['geom'].stride})"
    gts = [torch.zeros(pr["ref"].shape, device="cuda") for pr in prs]
    _finish(pkg, lib, [(pr, grp, sp, GSCALE, gt) for (pr, grp, sp), gt in zip(groups, gts)], False)
    torch.cuda.synchronize()
    worst = max(_check_sum(f"grouped wgrad {i}", gt, pr["ref"], pr["terms"]) for i, (pr, gt) in enumerate(zip(prs, gts)))
    _log(f"wgrad grouped n={n} {_name(T16)}", {"worst": worst})


# ---------------------------------------------------------------------------------------------------------------------
# 5. model-level switch consistency
# ---------------------------------------------------------------------------------------------------------------------

SETTINGS = {          # fields of resnet.TowerOptions that leave their default
    "fused": {},
    "bn_bwd_fuse=0": {"bn_bwd_fuse": False},
    "bn_bwd_fuse_out=0": {"block_out_fuse": False},
    "strided_dgrad=0": {"strided_dgrad": False},
    "wgrad_group=1": {"wgrad_group": 1},
    "all_off": {"bn_bwd_fuse": False, "block_out_fuse": False, "strided_dgrad": False, "wgrad_group": 1},
}
ACT_ULPS = 4           # activation gradients: max |a - b| in ulps (EPS) of the tensor's largest element
PARAM_REL_EPS = 10     # parameter gradients: ||a - b|| / ||b|| <= 10 EPS (fp16 9.8e-3, bf16 7.8e-2).  A BatchNorm bias gradient is a
                       # sum over B*H*W rows whose terms cancel to ~1/40 of their absolute sum, so the 1-ulp activation differences
                       # of another summation order show up ~40x larger in it than in the activations


def _instrument(monkeypatch, pkg, lib, T16, rec):
    """wrap the library entry points _backward_tape calls: record which fusions fire, copy the gradient entering and
    leaving the max pool (the tower's activation gradients; the image itself gets none)"""
    real = {n: getattr(lib, n) for n in ("mh_conv_dgrad", "mh_bn2d_bwd_parts", "mh_conv_wgrad", "mh_conv_wgrad_grouped", "mh_maxpool_bwd",
                                         "mh_add_h16")}

    def dgrad(dy, wk, dx, ws, geom, fuse, stream):
        if fuse is None:
            rec["dgrad_plain"] += 1
        elif fuse.addend is not None and fuse.y_mask is not None:
            rec["block_out"] += 1
        elif fuse.addend is None and fuse.y_mask is None:
            rec["fuse_prev"] += 1
        else:
            rec["other"] += 1
        if geom.stride == 2:
            rec["strided_dgrad"] += 1
        return real["mh_conv_dgrad"](dy, wk, dx, ws, geom, fuse, stream)

    def parts(*a):
        rec["pre_part"] += 1
        return real["mh_bn2d_bwd_parts"](*a)

    def wgrad(*a):
        rec["wgrad_single"] += 1
        return real["mh_conv_wgrad"](*a)

    def wgrad_grouped(*a):
        rec["wgrad_grouped"] += 1
        return real["mh_conv_wgrad_grouped"](*a)

    def copy16(ptr, n, stream):
        out = torch.empty(n, dtype=T16, device="cuda")
        zero = torch.zeros(n, dtype=T16, device="cuda")
        pkg._lib.check(real["mh_add_h16"](ptr, zero.data_ptr(), out.data_ptr(), n, stream), "copy")      # x + 0 = x
        return out

    def maxpool_bwd(dy, arg, dx, B, H, W, C, K, s, p, stream):
        st = real["mh_maxpool_bwd"](dy, arg, dx, B, H, W, C, K, s, p, stream)
        Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        rec["act"] = (copy16(dy, B * Ho * Wo * C, stream), copy16(dx, B * H * W * C, stream))
        return st

    monkeypatch.setattr(lib, "mh_conv_dgrad", dgrad)
    monkeypatch.setattr(lib, "mh_bn2d_bwd_parts", parts)
    monkeypatch.setattr(lib, "mh_conv_wgrad", wgrad)
    monkeypatch.setattr(lib, "mh_conv_wgrad_grouped", wgrad_grouped)
    monkeypatch.setattr(lib, "mh_maxpool_bwd", maxpool_bwd)


@DTYPES
def test_model_switches_agree(pkg, monkeypatch, T16):
    dtype = _name(T16)
    lib = _lib(pkg, T16)
    net = pkg.ResNet50(num_classes=10, compute_dtype=dtype, layers=(2, 1, 1, 1), seed=3).cuda().train()
    g = torch.Generator().manual_seed(800)
    image = torch.randn((4, 3, 64, 64), generator=g).cuda()
    R = (torch.randn((4, net.feature_dim), generator=g) * 1e-3).cuda()      # d_pooled of the size a loss gives
    rec = {}
    _instrument(monkeypatch, pkg, lib, T16, rec)
    results = {}
    for name, fields in SETTINGS.items():
        net.options = pkg.resnet.TowerOptions(**fields)
        rec.clear()
        rec.update({k: 0 for k in ("dgrad_plain", "block_out", "fuse_prev", "other", "strided_dgrad", "pre_part", "wgrad_single",
                                   "wgrad_grouped")})
        net.zero_grad(set_to_none=True)
        (net.features(image) * R).sum().backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if not n.startswith("fc.")}
        assert all(v is not None and bool(torch.isfinite(v).all()) for v in grads.values()), name
        assert all(bool(torch.isfinite(a).all()) for a in rec["act"]), name
        results[name] = (grads, tuple(a.float() for a in rec["act"]), dict(rec))
    counts = {n: r[2] for n, r in results.items()}
    c = counts["fused"]
    assert c["block_out"] == 4 and c["fuse_prev"] > 0 and c["pre_part"] > 0 and c["strided_dgrad"] == 3 and c["wgrad_grouped"] > 0, c
    assert c["other"] == 0 and c["wgrad_single"] == 0, c
    assert counts["bn_bwd_fuse=0"]["block_out"] == counts["bn_bwd_fuse=0"]["fuse_prev"] == counts["bn_bwd_fuse=0"]["pre_part"] == 0
    assert counts["bn_bwd_fuse_out=0"]["block_out"] == 0 and counts["bn_bwd_fuse_out=0"]["fuse_prev"] > 0
    assert counts["strided_dgrad=0"]["strided_dgrad"] == 0 and counts["strided_dgrad=0"]["block_out"] == 4
    assert counts["wgrad_group=1"]["wgrad_grouped"] == 0 and counts["wgrad_group=1"]["wgrad_single"] > 0
    assert counts["all_off"]["block_out"] + counts["all_off"]["fuse_prev"] + counts["all_off"]["pre_part"] + counts["all_off"]["wgrad_grouped"] == 0
    ref_grads, ref_act, _ = results["fused"]
    eps16 = _eps(T16)
    for name, (grads, act, _) in results.items():
        if name == "fused":
            continue
        worst_p, worst_name = 0.0, None
        for n, gr in grads.items():
            rr = ref_grads[n]
            rel = float((gr - rr).norm() / rr.norm().clamp_min(1e-30))
            if rel > worst_p:
                worst_p, worst_name = rel, n
        e_act = [float((a - b).abs().max()) / (eps16 * float(b.abs().max())) for a, b in zip(act, ref_act)]
        parity_log(f"[resnet model {dtype} {name} vs fused] param rel {worst_p:.3e} ({worst_name}) act ulps {e_act[0]:.2f} / {e_act[1]:.2f}")
        assert worst_p <= PARAM_REL_EPS * eps16, f"{name}: {worst_name} differs from the fused path by {worst_p:.3g} (relative norm)"
        assert max(e_act) <= ACT_ULPS, f"{name}: activation gradients differ from the fused path by {e_act} ulps of their maximum"
