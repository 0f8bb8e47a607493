"""Every head, loss, pooling and optimizer kernel (csrc/head.hip, csrc/smallops.hip, csrc/optim.hip) against one plain reference:
float64 torch on the CPU, computed from the same f32 (or 16-bit) tensors the kernels read.

The reference rounds to 16 bits exactly where a kernel stores 16 bits, and to f32 where the reproduced PyTorch module itself
works in f32 (attention pooling adds (1 - mask) * -1e9 to its f32 scores: the reference does that addition in f32 too, which is
what makes a fully masked row uniform).  Dropout masks are read back with ops.dropout_mask and injected into the reference.
Where a stage reads the output of an earlier one, its reference is computed from the KERNEL's earlier output (read back): every
bar then covers one stage's arithmetic only.

  case                                   kernel / template instance / host path
  ----------------------------------------------------------------------------------------------------------------------------
  gemm_f32 <layout> <variant>            gemm_f32_kernel<LA, LB, FAST> for (LA, LB) = 00 / 01 / 10 / 11; variant "tight" reaches
                                           FAST (16-B rows, K % 4 == 0; never for 11), "ldpad" (lda % 4 != 0) and "offset" (base
                                           1 float off 16-B alignment) force the bounded loads; K in {1 3 4 31 32 33 127 128 129
                                           2048} (the PF = 4 prefetch groups and the tiles past K), M / N in {1 63 64 65 130};
                                           TANH / RELU / ACCUM alone and combined; operand padding holds NaN (a read past K
                                           poisons C); rows >= M and columns [N, ldc) keep their sentinel
  gemm_f32_int <layout> <variant>        the same instances on small-integer operands: C == the exact sum bit for bit
  gemm_f32_bn M<m> <mode>                the fused BatchNorm1d epilogue: M in {1 2 63 64}, training / eval, gamma / beta NULL,
                                           RELU, z with ldz > N, N = 130 (a partial last column tile); sentinels past N in
                                           save_mean / save_rstd / running stats / z; running stats == nn.BatchNorm1d's update
  head <case>                            mh_head_fwd / mh_head_bwd (pool_kernel, linear_fwd_kernel, head_bwd_stage_kernel): the
                                           headline shape (B 32, S 128, Nt 197, Dt = Di 768, P 512, C 2) and B in {1 31 32 33 65}
                                           around the RB = 32 row block, Dt / Di not multiples of 64, C in {1 3}, pool 0 / S-1,
                                           dropout, text_rows (packed), out_scale != 1; both libraries (16-bit hidden grads)
  pool_standalone                        mh_pool_fwd / mh_pool_bwd, plain and text_rows
  ce B<b> C<c>                           ce_kernel: B in {1 63 64 65 1024}, C in {1 2 5 1000}, offsets +-1e4, argmax ties,
                                           grad_scale x grad_scale_dev; out-of-range labels (-100, C, 7C) read as class 0
  focal a<alpha> g<gamma>                focal_kernel: alpha {0.25 0 -1} x gamma {0 0.5 2 3}, |x| <= 30, targets 0 / 1 / 0.3
  bn1d B<b> F<f>                         bn1d_fwd_kernel / bn1d_bwd_kernel: B {1 2 1024} x F {1 255 256 257}, |mean|/std to 1e3,
                                           ReLU, frozen statistics, eval mode; B = 1 training: output beta, running var (1-mom) rv
  pool_max / pool_mean                   pool_max_{fwd,bwd}_kernel (ties: first max; NaN propagates as torch.max; S = 1),
                                           pool_mean_{fwd,bwd}_kernel (an all-zero mask row gives 0)
  pool_attn S<s> A<a>                    pool_attn_{fwd,bwd}_kernel: S {1 255 256 257 1024}, A {64 300}, D = 200, a fully masked row
  conv_pool taps<k>                      mh_pad_seq_f32, relu_max_{fwd,bwd}, mh_conv_fold_f32: taps {1 3 5 7}, S < taps, all
                                           pre-activations <= 0 (arg = -1, zero gradients)
  softmax_gate F<f>                      softmax_gate_{fwd,bwd}_kernel: F {1 63 64 65 1536}, logits offset by 1e4
  mca3 B<b>                              mca3_fwd_kernel, mca3_bwd_i_kernel, mca3_bwd_j_kernel: B {1 2 255 256 257 1024}, U = 72
  fused_autograd <op>                    the fused.py autograd Functions (the same kernels plus their mh_gemm_f32 / mh_colsum_f32
                                           glue) against float64 autograd of the reference formula
  colsum rows<r>                         colsum_f32_kernel: rows 1..5, D {1 63 64 65}, ld > D, scale != 1
  sumsq n<n>                             sumsq_part_kernel + sumsq_final_kernel: n {1..5, 4k+3}, many workgroups, n > 2^23 (1024
                                           partials)
  adam <case>                            adam_kernel: n {4, 8, 4k, > 2 097 152 (two grid-stride trips)}, n_shadow {0, < n, n},
                                           Adam-L2 / AdamW, grad_scale != 1 and < 0, max_norm with clip_norm_mult 0 / > 0,
                                           a non-finite norm, several steps with state carried; both libraries (shadow)
  adam_guarded                           the guarded form: an earlier ordinal's mark makes the launch a no-op; its own mark skips
                                           exactly the 4-element vectors whose gradient is not finite
  adam_rows D<d> rows<r>                 adam_rows_kernel: D {4 8 260 768}, rows {1 5 30522}, row_touched NULL, dead rows untouched,
                                           all rows live == adam_kernel bit for bit, the guarded form
  adam_skip_account                      adam_skip_account_kernel: a scripted clean / overflowing sequence against a Python
                                           GradScaler.update + bias-correction model, 1 - 8 groups, growth_interval 1 / 3, the
                                           min / max clamps, the overflow word cleared, gnorm_sq NULL
  cast / sum_shards                      cast_f32_bf16_kernel, cast_bf16_f32_kernel, sum_shards_kernel in both libraries

Bars (EPS32 = 2^-24, TOL_SUM = 1e-5, EPS = the 16-bit epsilon):
  * f32 sums and dot products: |hip - ref| <= TOL_SUM x sum|terms| (the float64 sum of the absolute terms behind the value);
  * tanhf / expf / logf / powf results add 8 EPS32 x |result| (OCML's f32 transcendental functions are within a few ulp);
  * stored 16-bit values: 1 ulp(ref) plus the f32 bar of the value before rounding;
  * short f32 formulas (BatchNorm apply, running statistics, one Adam update, the clip coefficient): 32 EPS32 x the sum of the
    absolute values of the formula's terms (at most ~16 roundings along the chain, 2x margin);
  * softmax-weighted outputs (attention pooling, MCA3, CE, the gate): the weights' bar is 2 p x (the bar of the logits) plus
    the normaliser's f32 sum bar, and every later stage is checked against the kernel's own weights;
  * statistics: mean within TOL_SUM x sum|x| / B; rstd relative within (TOL_SUM + (mean bar / std)^2) / 2 + 4 EPS32;
  * fused.py autograd chains (2 - 4 kernels each): |hip - ref| <= 1e-4 x max|ref| of the tensor (each stage is held to its own
    TOL_SUM bar in the stand-alone cases; 1e-4 covers four such stages whose terms are up to 2.5x the output's scale);
  * bit-exact: copies, casts (== torch .to(), NaN payloads compared as NaN), integer sums, max, the same formula on the same
    inputs (all-live rows == the dense Adam, guarded == unguarded off the skipped vectors, skip_account's f32 scalars), and all
    memory a kernel must not write (sentinels).
Measured worst errors go through conftest.parity_log (profiles/r07_head_optim_paths_parity.txt): each as a fraction of its bar.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import parity_log

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64, I16, I32, I64, U8 = (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int16, torch.int32,
                                          torch.int64, torch.uint8)
DTYPES = pytest.mark.parametrize("T16", [F16, BF16], ids=["fp16", "bf16"])
MANT = {F16: 10, BF16: 7}
EMIN = {F16: -14, BF16: -126}
EPS32 = 2.0 ** -24
TOL_SUM = 1e-5
TRANS = 8 * EPS32        # f32 transcendental functions, relative
FORM = 32 * EPS32        # short f32 formulas, relative to the sum of |terms|
COMP = 1e-4              # fused.py autograd chains, relative to max|ref|
SENT16 = 0x7BAD
SENT32 = -7777.0
F32_TANH, F32_RELU, F32_ACCUM, F32_BN = 2, 4, 1, 8


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_num_threads(16)
    import multimodal_propaganda_meme_classification_amd as m
    from multimodal_propaganda_meme_classification_amd import fused as _fused
    from multimodal_propaganda_meme_classification_amd import ops as _ops
    m.ops, m.fused = _ops, _fused
    yield m
    torch.cuda.synchronize()
    torch.cuda.empty_cache()        # the sumsq / Adam cases cache ~1 GB of blocks: hand them back before the next module


def _lib(pkg, T16=BF16):
    return pkg._lib.load("fp16" if T16 == F16 else "bf16")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(pkg, status, what):
    pkg._lib.check(status, what)


def _name(T16):
    return "fp16" if T16 == F16 else "bf16"


def _ulp(ref, T16):
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** EMIN[T16]))
    return torch.pow(2.0, (e - 1 - MANT[T16]).to(F64))


def _cpu(t):
    return t.detach().cpu().to(F64)


def _f32(t64):
    """float64 -> the f32 value a kernel reads, as float64"""
    return t64.to(F32).to(F64)


def _dev32(t64):
    return t64.to(F32).cuda().contiguous()


def _rand(shape, g, scale=1.0, shift=0.0):
    return _f32(torch.randn(shape, generator=g, dtype=F64) * scale + shift)


def _ints(shape, g, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _sent16(n, T16):
    return torch.full((n,), SENT16, dtype=I16, device="cuda").view(T16)


def _bits(t):
    return t.view(I16) if t.element_size() == 2 else t.view(I32)


def _same_bits(a, b):
    return torch.equal(_bits(a.detach().cpu().contiguous()), _bits(b.detach().cpu().contiguous()))


def _check(what, got, ref, bar):
    """|got - ref| <= bar elementwise.  Returns the worst error as a fraction of the bar."""
    got = _cpu(got).reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
    bar = torch.as_tensor(bar, dtype=F64).expand_as(ref) + 1e-37
    frac = (got - ref).abs() / bar
    worst = float(frac.max()) if frac.numel() else 0.0
    if worst > 1.0:
        i = int(frac.argmax())
        raise AssertionError(f"{what}: {int((frac > 1).sum())}/{frac.numel()} off; worst {worst:.3g} x bar (ref "
                             f"{float(ref.flatten()[i]):.6g}, got {float(got.flatten()[i]):.6g}, bar {float(bar.flatten()[i]):.3g})")
    return worst


def _check16(what, got, ref, T16, slack):
    return _check(what, got, ref, _ulp(ref, T16) + slack)


def _comp(what, got, ref):
    return _check(what, got, ref, COMP * float(ref.abs().max()) + 1e-30)


def _log(tag, errs):
    parity_log(f"[headopt {tag}] " + " ".join(f"{k} {x:.3e}" if isinstance(x, float) else f"{k} {x}" for k, x in errs.items()))


def _drop(seed, p, site):
    return (torch.tensor([seed & 0x7FFFFFFF, 0, 5, 0], dtype=I32, device="cuda"), p, site)


def _drop_scale(p):
    return float(torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. mh_gemm_f32
# ---------------------------------------------------------------------------------------------------------------------------------

F32_LAYOUTS = pytest.mark.parametrize("layout", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["00", "01", "10", "11"])
F32_VARIANTS = pytest.mark.parametrize("variant", ["tight", "ldpad", "offset"])
MN_PAIRS = [(1, 130), (63, 65), (64, 64), (65, 1), (130, 63)]
KS = [1, 3, 4, 31, 32, 33, 127, 128, 129, 2048]
FLAG_CYCLE = [0, F32_TANH, F32_RELU, F32_ACCUM, F32_TANH | F32_ACCUM, F32_RELU | F32_ACCUM, F32_TANH | F32_RELU]


def _operand(X, kmajor, variant):
    """X logical [R][K] (float64 of f32 values) -> (device buffer, float offset, ld, vec): stored [R][ld] or [K][ld], padding NaN"""
    R, K = X.shape
    rows, cols = (K, R) if kmajor else (R, K)
    off = 1 if variant == "offset" else 0
    if variant == "tight":
        ld = cols
    elif variant == "ldpad":
        ld = cols + 1 if (cols + 1) % 4 else cols + 2
    else:
        ld = (cols + 3) // 4 * 4
    buf = torch.full((off + rows * ld + 8,), float("nan"), dtype=F32)
    buf[off:off + rows * ld].view(rows, ld)[:, :cols] = (X.t() if kmajor else X).to(F32)
    vec = ld % 4 == 0 and off == 0
    return buf.cuda(), off, ld, vec


def _gemm_f32_raw(pkg, A, a_off, lda, B, b_off, ldb, Cbuf, ldc, M, N, K, la, lb, bias=None, flags=0, bn=None):
    p = pkg._lib.MhGemmF32()
    p.A, p.B, p.C = A.data_ptr() + 4 * a_off, B.data_ptr() + 4 * b_off, Cbuf.data_ptr()
    p.bias = None if bias is None else bias.data_ptr()
    p.M, p.N, p.K, p.lda, p.ldb, p.ldc, p.flags = M, N, K, lda, ldb, ldc, flags
    if bn is not None:
        p.flags |= F32_BN
        for fld, key in (("bn_gamma", "gamma"), ("bn_beta", "beta"), ("bn_running_mean", "rm"), ("bn_running_var", "rv"),
                         ("bn_save_mean", "sm"), ("bn_save_rstd", "sr"), ("bn_z", "z")):
            t = bn.get(key)
            setattr(p, fld, None if t is None else t.data_ptr())
        p.bn_ldz, p.bn_eps, p.bn_momentum, p.bn_training = bn["ldz"], bn["eps"], bn["momentum"], int(bn["training"])
    _ok(pkg, _lib(pkg).mh_gemm_f32(C.byref(p), la, lb, _st()), "mh_gemm_f32")


def _is_fast(K, la, lb, va, vb):
    return K % 4 == 0 and (la or va) and (lb or vb) and not (la and lb)


def _run_f32_case(pkg, layout, variant, M, N, K, A, B, bias, flags, C0):
    la, lb = layout
    Ad, ao, lda, va = _operand(A, la, variant)
    Bd, bo, ldb, vb = _operand(B, lb, variant)
    ldc = N + 3
    Cfull = torch.full((M + 2, ldc), SENT32, dtype=F32)
    if C0 is not None:
        Cfull[:M, :N] = C0.to(F32)
    Cd = Cfull.cuda()
    _gemm_f32_raw(pkg, Ad, ao, lda, Bd, bo, ldb, Cd, ldc, M, N, K, la, lb,
                  bias=None if bias is None else _dev32(bias), flags=flags)
    Cg = Cd.cpu()
    keep = torch.ones_like(Cg, dtype=torch.bool)
    keep[:M, :N] = False
    assert bool((Cg[keep] == SENT32).all()), f"gemm_f32 {layout} {variant} M{M} N{N} K{K}: wrote outside [M) x [N)"
    return Cg[:M, :N].to(F64), _is_fast(K, la, lb, va, vb)


def _f32_ref(A, B, bias, flags, C0):
    acc = A @ B.t()
    terms = A.abs() @ B.abs().t()
    if bias is not None:
        acc = acc + bias
        terms = terms + bias.abs()
    extra = torch.zeros_like(acc)
    if flags & F32_TANH:
        acc = torch.tanh(acc)
        extra = TRANS * acc.abs()
    if flags & F32_RELU:
        acc = acc.clamp_min(0.0)
    if flags & F32_ACCUM:
        acc = acc + C0
        terms = terms + C0.abs()
    return acc, TOL_SUM * terms + extra


@F32_LAYOUTS
@F32_VARIANTS
def test_gemm_f32_paths(pkg, layout, variant):
    g = torch.Generator().manual_seed(100 + 10 * layout[0] + layout[1])
    worst, nfast, nslow, case = 0.0, 0, 0, 0
    for K in KS:
        for M, N in MN_PAIRS:
            flags = FLAG_CYCLE[case % len(FLAG_CYCLE)]
            A, B = _rand((M, K), g), _rand((N, K), g, 1.0 / math.sqrt(K))
            bias = _rand((N,), g, 0.5) if case % 2 == 0 else None
            C0 = _rand((M, N), g) if flags & F32_ACCUM else None
            got, fast = _run_f32_case(pkg, layout, variant, M, N, K, A, B, bias, flags, C0)
            ref, bar = _f32_ref(A, B, bias, flags, C0)
            worst = max(worst, _check(f"gemm_f32 {layout} {variant} M{M} N{N} K{K} flags{flags}", got, ref, bar))
            nfast += fast
            nslow += not fast
            case += 1
    if variant == "tight" and layout != (1, 1):
        assert nfast >= 20, nfast           # FAST reached at every K % 4 == 0
    else:
        assert nfast == 0
    _log(f"gemm_f32 {layout[0]}{layout[1]} {variant}", {"C": worst, "fast_cases": nfast, "bounded_cases": nslow})


@F32_LAYOUTS
@F32_VARIANTS
def test_gemm_f32_int_exact(pkg, layout, variant):
    g = torch.Generator().manual_seed(200 + 10 * layout[0] + layout[1])
    n = 0
    for K in KS:
        for M, N in MN_PAIRS:
            flags = [0, F32_RELU, F32_ACCUM, F32_RELU | F32_ACCUM][n % 4]
            A, B = _ints((M, K), g, -3, 3), _ints((N, K), g, -3, 3)
            bias = _ints((N,), g, -50, 50)
            C0 = _ints((M, N), g, -100, 100) if flags & F32_ACCUM else None
            got, _ = _run_f32_case(pkg, layout, variant, M, N, K, A, B, bias, flags, C0)
            ref, _ = _f32_ref(A, B, bias, flags, C0)
            assert torch.equal(got, ref), f"gemm_f32 int {layout} {variant} M{M} N{N} K{K} flags{flags}"
            n += 1
    _log(f"gemm_f32_int {layout[0]}{layout[1]} {variant}", {"C": f"== exact sum bit for bit ({n} shapes)"})


BN_CASES = [(m, mode) for m in (1, 2, 63, 64) for mode in ("train", "train_relu_noaffine", "eval", "eval_relu")]


@pytest.mark.parametrize("M,mode", BN_CASES, ids=[f"M{m}_{mode}" for m, mode in BN_CASES])
def test_gemm_f32_bn_epilogue(pkg, M, mode):
    g = torch.Generator().manual_seed(300 + M)
    N, K, ldz = 130, (37 if M % 2 else 64), 133
    training, relu, affine = mode.startswith("train"), "relu" in mode, "noaffine" not in mode
    A, B = _rand((M, K), g), _rand((N, K), g, 1.0 / math.sqrt(K))
    bias = _rand((N,), g, 2.0)
    gamma, beta = _rand((N,), g, 0.5, 1.0), _rand((N,), g, 0.5)
    rm0, rv0 = _rand((N,), g, 0.5), _f32(torch.rand(N, generator=g, dtype=F64) + 0.5)
    mom, eps = 0.1, 1e-5

    def buf(v=None):
        t = torch.full((N + 5,), SENT32, dtype=F32)
        if v is not None:
            t[:N] = v.to(F32)
        return t.cuda()

    rm, rv, sm, sr = buf(rm0), buf(rv0), buf(), buf()
    z = torch.full((M * ldz + 4,), SENT32, dtype=F32, device="cuda")
    Ad, Bd = _dev32(A), _dev32(B)
    ldc = N + 3
    Cd = torch.full((M + 2, ldc), SENT32, dtype=F32, device="cuda")
    bn = dict(gamma=_dev32(gamma) if affine else None, beta=_dev32(beta) if affine else None, rm=rm, rv=rv, sm=sm, sr=sr, z=z,
              ldz=ldz, eps=eps, momentum=mom, training=training)
    _gemm_f32_raw(pkg, Ad, 0, K, Bd, 0, K, Cd, ldc, M, N, K, 0, 0, bias=_dev32(bias), flags=F32_RELU if relu else 0, bn=bn)
    torch.cuda.synchronize()
    for nm, t in (("save_mean", sm), ("save_rstd", sr), ("running_mean", rm), ("running_var", rv)):
        assert bool((t.cpu()[N:] == SENT32).all()), f"{nm}: columns >= N written"
    zz = z.cpu()[:M * ldz].view(M, ldz)
    assert bool((zz[:, N:] == SENT32).all()) and bool((z.cpu()[M * ldz:] == SENT32).all()), "z: columns [N, ldz) written"
    Cg = Cd.cpu()
    keep = torch.ones_like(Cg, dtype=torch.bool)
    keep[:M, :N] = False
    assert bool((Cg[keep] == SENT32).all()), "C: written outside [M) x [N)"
    errs = {}
    zk = zz[:, :N].to(F64)
    zref, zbar = _f32_ref(A, B, bias, 0, None)
    errs["z"] = _check("bn z", zk, zref, zbar)
    smk, srk = _cpu(sm[:N]), _cpu(sr[:N])
    ga, be = (gamma, beta) if affine else (torch.ones(N, dtype=F64), torch.zeros(N, dtype=F64))
    if training:
        mu = zk.mean(0)
        var = zk.var(0, unbiased=False)
        mbar = TOL_SUM * zk.abs().sum(0) / M
        errs["mean"] = _check("bn mean", smk, mu, mbar)
        rs = 1.0 / torch.sqrt(var + _f32(torch.tensor(eps, dtype=F64)))
        sd = torch.sqrt(var).clamp_min(1e-30)
        errs["rstd"] = _check("bn rstd", srk, rs, rs * (0.5 * (TOL_SUM + (mbar / sd) ** 2) + 4 * EPS32))
        if M > 1:
            ref_bn = torch.nn.BatchNorm1d(N, eps=eps, momentum=mom, dtype=F64)
            with torch.no_grad():
                ref_bn.running_mean.copy_(rm0)
                ref_bn.running_var.copy_(rv0)
            ref_bn.train()
            ref_bn(zk)
            errs["running_mean"] = _check("bn running_mean", rm[:N], ref_bn.running_mean.detach(),
                                          FORM * ((1 - mom) * rm0.abs() + mom * mu.abs()) + mom * mbar)
            uv = zk.var(0, unbiased=True)
            errs["running_var"] = _check("bn running_var", rv[:N], ref_bn.running_var.detach(),
                                         FORM * ((1 - mom) * rv0.abs() + mom * uv) + mom * uv * (TOL_SUM + (mbar / sd) ** 2))
        else:
            # documented divergence: nn.BatchNorm1d refuses one training row; the kernel normalises with variance 0 (output = beta)
            # and feeds the biased variance 0 into the running variance
            with pytest.raises(ValueError):
                torch.nn.BatchNorm1d(N, dtype=F64).train()(zk)
            assert torch.equal(smk, zk[0]), "M = 1: the mean is the row itself"
            assert torch.equal(_cpu(rv[:N]), _f32(_f32(1 - _f32(torch.tensor(mom, dtype=F64))) * rv0)), "M = 1: running var"
            want = be.clamp_min(0.0) if relu else be
            assert torch.equal(Cg[:1, :N].to(F64), want.reshape(1, N)), "M = 1: output != beta"
    else:
        assert torch.equal(smk, rm0) and torch.equal(_cpu(rm[:N]), rm0) and torch.equal(_cpu(rv[:N]), rv0)
        rs = 1.0 / torch.sqrt(rv0 + _f32(torch.tensor(eps, dtype=F64)))
        errs["rstd"] = _check("bn eval rstd", srk, rs, rs * 4 * EPS32)
    xh = (zk - smk) * srk
    y = xh * ga + be
    if relu:
        y = y.clamp_min(0.0)
    errs["y"] = _check("bn y", Cg[:M, :N].to(F64), y, FORM * ((xh * ga).abs() + be.abs()) + 1e-30)
    _log(f"gemm_f32_bn M{M} {mode}", errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. head (csrc/head.hip)
# ---------------------------------------------------------------------------------------------------------------------------------

HEAD_CASES = {   # name: (B, S, Nt, Dt, Di, P, C, pool, drop_p, packed, out_scale)
    "headline_B32_768_P512": (32, 128, 197, 768, 768, 512, 2, 0, 0.0, False, 1.0),
    "headline_drop_scale": (32, 128, 197, 768, 768, 512, 2, 0, 0.3, False, 1024.0),
    "B1_C1_pool0": (1, 16, 5, 100, 72, 64, 1, 0, 0.0, False, 1.0),
    "B31_C3_poolS-1": (31, 16, 5, 100, 72, 48, 3, 15, 0.0, False, 0.5),
    "B32_C3_drop": (32, 9, 3, 130, 190, 40, 3, 4, 0.3, False, 1.0),
    "B33_C1_packed": (33, 16, 5, 100, 72, 64, 1, 0, 0.0, True, 8.0),
    "B65_C3_packed_drop": (65, 12, 2, 200, 72, 33, 3, 0, 0.3, True, 2.0),
}


def _head_setup(case, seed):
    B, S, Nt, Dt, Di, P, Cn, pool, dp, packed, osc = HEAD_CASES[case]
    g = torch.Generator().manual_seed(seed)
    th = _rand((B * S, Dt), g)
    ih = _rand((B * Nt, Di), g)
    shapes = [(P, Dt), (P,), (P, Di), (P,), (P, 2 * P), (P,), (Cn, P), (Cn,)]
    params = [_rand(s, g, 0.5 / math.sqrt(s[-1] if len(s) == 2 else 4)) for s in shapes]
    rows = None
    if packed:      # text_rows: one arbitrary distinct row per sample (packed token rows)
        rows = torch.randperm(B * S, generator=g)[:B].to(I64)
    return (B, S, Nt, Dt, Di, P, Cn, pool, dp, packed, osc), th, ih, params, rows


@DTYPES
@pytest.mark.parametrize("case", list(HEAD_CASES))
def test_head_fwd_bwd(pkg, case, T16):
    (B, S, Nt, Dt, Di, P, Cn, pool, dp, packed, osc), th, ih, params, rows = _head_setup(case, 400 + list(HEAD_CASES).index(case))
    g = torch.Generator().manual_seed(7)
    pd = [_dev32(p) for p in params]
    drop = _drop(1234, dp, 41) if dp > 0 else None
    rows_d = None if rows is None else rows.to(I32).cuda()
    pooled = torch.empty((B, Dt + Di), dtype=F32, device="cuda")
    feat, fused, logits = (torch.empty(s, dtype=F32, device="cuda") for s in ((B, 2 * P), (B, P), (B, Cn)))
    pkg.ops.head_fwd(pd, _dev32(th), _dev32(ih), pool, pooled, feat, fused, logits, B, S, Nt, Dt, Di, P, Cn, drop=drop,
                     text_rows=rows_d)
    Wt, bt, Wi, bi, Wf, bf, Wo, bo = params
    trow = rows if rows is not None else torch.arange(B) * S + pool
    mask = torch.ones(B * Dt, dtype=F64)
    if drop is not None:
        mask = pkg.ops.dropout_mask(B * Dt, drop, "cuda").cpu().to(F64) * _drop_scale(dp)
        assert 0.5 < float((mask > 0).double().mean()) < 0.9
    mask = mask.view(B, Dt)
    pt_ref = _f32(th[trow] * mask)         # one f32 multiply: exact to the f32 rounding
    pk = _cpu(pooled)
    assert torch.equal(pk[:, :Dt], pt_ref) and torch.equal(pk[:, Dt:], ih.view(B, Nt, Di)[:, 0]), "pooled != gather (x mask)"
    errs = {}
    fk, fuk, lk = _cpu(feat), _cpu(fused), _cpu(logits)

    def lin(x, W, b):
        return x @ W.t() + b, TOL_SUM * (x.abs() @ W.abs().t() + b.abs())

    r1, b1 = lin(pk[:, :Dt], Wt, bt)
    r2, b2 = lin(pk[:, Dt:], Wi, bi)
    errs["feat"] = _check("feat", fk, torch.cat([r1, r2], 1), torch.cat([b1, b2], 1))
    errs["fused"] = _check("fused", fuk, *lin(fk, Wf, bf))
    errs["logits"] = _check("logits", lk, *lin(fuk, Wo, bo))
    # backward
    dl = _rand((B, Cn), g, 0.3)
    grads = [torch.empty_like(p) for p in pd]
    dfeat, dfused = torch.empty_like(feat), torch.empty_like(fused)
    dth = _sent16(B * S * Dt, T16).view(B * S, Dt)
    dih = _sent16(B * Nt * Di, T16).view(B * Nt, Di)
    pkg.ops.head_bwd(pd, grads, _dev32(dl), pooled, feat, fused, dfeat, dfused, dth, dih, pool, B, S, Nt, Dt, Di, P, Cn,
                     out_scale=osc, drop=drop, text_rows=rows_d)
    torch.cuda.synchronize()
    gk = [_cpu(t) for t in grads]
    dfuk, dfk = _cpu(dfused), _cpu(dfeat)

    def dw(dy, x):
        return dy.t() @ x, TOL_SUM * (dy.abs().t() @ x.abs())

    def db(dy):
        return dy.sum(0), TOL_SUM * dy.abs().sum(0)

    errs["dWo"] = _check("dWo", gk[6], *dw(dl, fuk))
    errs["dbo"] = _check("dbo", gk[7], *db(dl))
    errs["dfused"] = _check("dfused", dfuk, dl @ Wo, TOL_SUM * (dl.abs() @ Wo.abs()))
    errs["dWf"] = _check("dWf", gk[4], *dw(dfuk, fk))
    errs["dbf"] = _check("dbf", gk[5], *db(dfuk))
    errs["dfeat"] = _check("dfeat", dfk, dfuk @ Wf, TOL_SUM * (dfuk.abs() @ Wf.abs()))
    errs["dWt"] = _check("dWt", gk[0], *dw(dfk[:, :P], pk[:, :Dt]))
    errs["dbt"] = _check("dbt", gk[1], *db(dfk[:, :P]))
    errs["dWi"] = _check("dWi", gk[2], *dw(dfk[:, P:], pk[:, Dt:]))
    errs["dbi"] = _check("dbi", gk[3], *db(dfk[:, P:]))
    f = osc * mask
    xt = dfk[:, :P] @ Wt * f
    xi = dfk[:, P:] @ Wi * osc
    dthc, dihc = dth.cpu(), dih.cpu()
    errs["d_text_hidden"] = _check16("d_text_hidden", dthc[trow].to(F64), xt, T16,
                                     TOL_SUM * (dfk[:, :P].abs() @ Wt.abs()) * f.abs())
    icls = torch.arange(B) * Nt
    errs["d_image_hidden"] = _check16("d_image_hidden", dihc[icls].to(F64), xi, T16, TOL_SUM * (dfk[:, P:].abs() @ Wi.abs()) * osc)
    tkeep = torch.ones(B * S, dtype=torch.bool)
    tkeep[trow] = False
    ikeep = torch.ones(B * Nt, dtype=torch.bool)
    ikeep[icls] = False
    assert bool((dthc[tkeep].view(I16) == SENT16).all()), "d_text_hidden: a row other than the pooled ones was written"
    assert bool((dihc[ikeep].view(I16) == SENT16).all()), "d_image_hidden: a row other than the class tokens was written"
    _log(f"head {case} {_name(T16)}", errs)


@DTYPES
@pytest.mark.parametrize("packed", [False, True], ids=["plain", "text_rows"])
def test_pool_standalone(pkg, packed, T16):
    B, S, Nt, Dt, Di, pool = 33, 7, 3, 70, 130, 6
    g = torch.Generator().manual_seed(500 + packed)
    th, ih = _rand((B * S, Dt), g), _rand((B * Nt, Di), g)
    rows = torch.randperm(B * S, generator=g)[:B] if packed else torch.arange(B) * S + pool
    rows_d = rows.to(I32).cuda() if packed else None
    pooled = torch.full((B, Dt + Di), SENT32, dtype=F32, device="cuda")
    L = _lib(pkg, T16)
    thd, ihd = _dev32(th), _dev32(ih)
    _ok(pkg, L.mh_pool_fwd(thd.data_ptr(), ihd.data_ptr(), pool, pooled.data_ptr(), B, S, Nt, Dt, Di,
                           None if rows_d is None else rows_d.data_ptr(), _st()), "mh_pool_fwd")
    want = torch.cat([th[rows], ih.view(B, Nt, Di)[:, 0]], 1)
    assert torch.equal(_cpu(pooled), want)
    dp = _rand((B, Dt + Di), g, 3.0)
    dth, dih = _sent16(B * S * Dt, T16).view(B * S, Dt), _sent16(B * Nt * Di, T16).view(B * Nt, Di)
    scale = 0.375
    dpd = _dev32(dp)
    _ok(pkg, L.mh_pool_bwd(dpd.data_ptr(), dth.data_ptr(), dih.data_ptr(), pool, B, S, Nt, Dt, Di, scale,
                           None if rows_d is None else rows_d.data_ptr(), _st()), "mh_pool_bwd")
    torch.cuda.synchronize()
    dthc, dihc = dth.cpu(), dih.cpu()
    # one f32 multiply by 0.375 (3 x 2^-3: exact) then one 16-bit rounding: == torch's .to() bit for bit
    assert _same_bits(dthc[rows], (dp[:, :Dt] * scale).to(T16))
    icls = torch.arange(B) * Nt
    assert _same_bits(dihc[icls], (dp[:, Dt:] * scale).to(T16))
    tk = torch.ones(B * S, dtype=torch.bool)
    tk[rows] = False
    ik = torch.ones(B * Nt, dtype=torch.bool)
    ik[icls] = False
    assert bool((dthc[tk].view(I16) == SENT16).all()) and bool((dihc[ik].view(I16) == SENT16).all())
    _log(f"pool_standalone {'text_rows' if packed else 'plain'} {_name(T16)}", {"pooled / d_hidden": "bit-exact, sentinels kept"})


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. losses
# ---------------------------------------------------------------------------------------------------------------------------------

CE_CASES = [(b, c) for b in (1, 63, 64, 65, 1024) for c in (1, 2, 5, 1000)]


def _ce_ref(z, y, inv):
    """float64 loss / dlogits of the f32 logits z, with the bars of the kernel's f32 evaluation (see the module docstring)"""
    B, Cn = z.shape
    mx = z.max(1).values
    lse = mx + torch.log(torch.exp(z - mx[:, None]).sum(1))
    zy = z[torch.arange(B), y]
    li = lse - zy
    lse_bar = 4 * EPS32 * (mx.abs() + (lse - mx).abs()) + (Cn + 4) * EPS32
    lbar = 4 * EPS32 * zy.abs() + lse_bar
    loss = li.mean()
    loss_bar = float(lbar.mean() + (B + 2) * EPS32 * li.abs().mean())
    p = torch.exp(z - lse[:, None])
    oh = torch.zeros_like(z)
    oh[torch.arange(B), y] = 1.0
    d = (p - oh) * inv
    dbar = abs(inv) * (p * (2 * EPS32 * (z.abs() + lse.abs()[:, None]) + lse_bar[:, None] + TRANS) + 2 * EPS32 * (p - oh).abs())
    return loss, loss_bar, d, dbar


@pytest.mark.parametrize("B,Cn", CE_CASES, ids=[f"B{b}_C{c}" for b, c in CE_CASES])
def test_ce(pkg, B, Cn):
    g = torch.Generator().manual_seed(600 + B + Cn)
    errs = {}
    for k, (offset, ties) in enumerate(((0.0, False), (1e4, False), (-1e4, False), (0.0, True))):
        if ties:        # small integers: many argmax ties, first index must win
            z = _ints((B, Cn), g, 0, 2)
        else:
            z = _rand((B, Cn), g, 3.0, offset)
        y = torch.randint(0, Cn, (B,), generator=g)
        gs, gsd = (1.0, None) if k % 2 == 0 else (0.75, 96.0)
        zd, yd = _dev32(z), y.cuda()
        loss = torch.empty(1, dtype=F32, device="cuda")
        dl = torch.full((B, Cn), SENT32, dtype=F32, device="cuda")
        nc = torch.empty(1, dtype=I32, device="cuda")
        pkg.ops.ce_fwd_bwd(zd, yd, loss, dl, nc, grad_scale=gs,
                           grad_scale_dev=None if gsd is None else torch.tensor([gsd], dtype=F32, device="cuda"))
        gs32 = np.float32(gs) * (np.float32(gsd) if gsd is not None else np.float32(1))
        inv = float(np.float32(gs32) / np.float32(B))
        loss_r, lbar, d_r, dbar = _ce_ref(z, y, inv)
        tag = f"off{offset:g}" + ("_ties" if ties else "") + ("_gsdev" if gsd else "")
        errs[f"loss_{tag}"] = _check(f"ce loss {tag}", loss, loss_r.reshape(1), lbar)
        errs[f"dlogits_{tag}"] = _check(f"ce dlogits {tag}", dl, d_r, dbar)
        assert int(nc) == int((z.argmax(1) == y).sum()), f"n_correct {tag}"      # torch.argmax: first maximal index
    # documented divergence: a label outside [0, C) (ignore_index -100 included) is read as class 0
    z = _rand((B, Cn), g, 2.0)
    bad = torch.tensor([-100, Cn, 7 * Cn, -1], dtype=I64)[torch.arange(B) % 4]
    outs = []
    for lab in (bad, torch.zeros(B, dtype=I64)):
        loss = torch.empty(1, dtype=F32, device="cuda")
        dl = torch.empty((B, Cn), dtype=F32, device="cuda")
        nc = torch.empty(1, dtype=I32, device="cuda")
        pkg.ops.ce_fwd_bwd(_dev32(z), lab.cuda(), loss, dl, nc)
        outs.append((loss.cpu(), dl.cpu(), nc.cpu()))
    assert all(_same_bits(a, b) for a, b in zip(outs[0], outs[1])), "an out-of-range label is not read as class 0"
    _log(f"ce B{B} C{Cn}", errs)


FOCAL_CASES = [(a, gm) for a in (0.25, 0.0, -1.0) for gm in (0.0, 0.5, 2.0, 3.0)]


@pytest.mark.parametrize("alpha,gamma", FOCAL_CASES, ids=[f"a{a:g}_g{gm:g}" for a, gm in FOCAL_CASES])
def test_focal(pkg, alpha, gamma):
    g = torch.Generator().manual_seed(700 + int(10 * gamma) + int(100 * alpha))
    B = 999
    x = _f32(torch.cat([torch.tensor([-30.0, 30.0, 0.0, -17.0, 17.0, 1e-3], dtype=F64), (torch.rand(B - 6, generator=g, dtype=F64) * 60 - 30)]))
    t = _f32(torch.tensor([0.0, 1.0, 0.3], dtype=F64))[torch.randint(0, 3, (B,), generator=g)]
    gs = 4.0
    loss = torch.empty(1, dtype=F32, device="cuda")
    dl = torch.empty(B, dtype=F32, device="cuda")
    nc = torch.empty(1, dtype=I32, device="cuda")
    pkg.ops.focal_fwd_bwd(_dev32(x), _dev32(t), loss, dl, nc, alpha=alpha, gamma=gamma, grad_scale=gs)
    # torchvision.ops.sigmoid_focal_loss (reduction "mean") in float64, through autograd
    xr = x.clone().requires_grad_(True)
    p = torch.sigmoid(xr)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(xr, t, reduction="none")
    pt = p * t + (1 - p) * (1 - t)
    lb = ce * ((1 - pt) ** gamma)
    at = alpha * t + (1 - alpha) * (1 - t) if alpha >= 0 else torch.ones_like(t)
    lb = at * lb
    (lb.mean() * gs).backward()
    # bars: 16 EPS32 relative to each term; p carries an absolute f32 error of a few EPS32, which moves the loss and its gradient
    # by at most (1 + gamma) |at| (1 + ce) times it
    with torch.no_grad():
        om = 1 - pt
        absf = 4 * EPS32 * (1 + gamma) * at.abs() * (1 + ce)
        lbar = float(((16 * EPS32 * lb.abs() + absf).sum() + B * EPS32 * lb.abs().sum()) / B)
        dce = (p - t)
        dmod = -gamma * om ** (gamma - 1) * (2 * t - 1) * p * (1 - p) if gamma > 0 else torch.zeros_like(t)
        gterms = at.abs() * ((dce * om ** gamma).abs() + (ce * dmod).abs())
        gbar = (16 * EPS32 * gterms + absf) * gs / B
    errs = {"loss": _check("focal loss", loss, lb.mean().detach().reshape(1), lbar),
            "dlogits": _check("focal dlogits", dl, xr.grad, gbar)}
    assert int(nc) == int(((x > 0) == (t > 0.5)).sum())
    _log(f"focal a{alpha:g} g{gamma:g}", errs)


BN1D_CASES = [(b, f) for b in (1, 2, 1024) for f in (1, 255, 256, 257)]


@pytest.mark.parametrize("B,Fn", BN1D_CASES, ids=[f"B{b}_F{f}" for b, f in BN1D_CASES])
def test_bn1d(pkg, B, Fn):
    g = torch.Generator().manual_seed(800 + B + Fn)
    mu_t = torch.tensor([0.0, 10.0, 1e3, -1e3], dtype=F64)[torch.arange(Fn) % 4]     # |mean| / std up to 1e3
    x = _f32(torch.randn(B, Fn, generator=g, dtype=F64) + mu_t)
    gamma, beta = _rand((Fn,), g, 0.5, 1.0), _rand((Fn,), g, 0.5)
    rm0, rv0 = _rand((Fn,), g, 0.5), _f32(torch.rand(Fn, generator=g, dtype=F64) + 0.5)
    eps, mom = 1e-5, 0.1
    eps32 = float(_f32(torch.tensor(eps, dtype=F64)))
    errs = {}
    for mode in ("train", "train_relu", "eval", "eval_relu"):
        training, relu = mode.startswith("train"), mode.endswith("relu")
        rm, rv = _dev32(rm0), _dev32(rv0)
        y, sm, sr = pkg.ops.bn1d_fwd(_dev32(x), _dev32(gamma), _dev32(beta), rm, rv, eps, mom, training, relu)
        smk, srk = _cpu(sm), _cpu(sr)
        if training:
            mu, var = x.mean(0), x.var(0, unbiased=False)
            mbar = TOL_SUM * x.abs().sum(0) / B
            errs[f"{mode}_mean"] = _check(f"bn1d {mode} mean", smk, mu, mbar)
            rs = 1 / torch.sqrt(var + eps32)
            sd = torch.sqrt(var).clamp_min(1e-30)
            errs[f"{mode}_rstd"] = _check(f"bn1d {mode} rstd", srk, rs, rs * (0.5 * (TOL_SUM + (mbar / sd) ** 2) + 4 * EPS32))
            errs[f"{mode}_running_mean"] = _check("running_mean", rm, (1 - mom) * rm0 + mom * smk,
                                                  FORM * ((1 - mom) * rm0.abs() + mom * smk.abs()))
            if B > 1:
                uv = x.var(0, unbiased=True)
                errs[f"{mode}_running_var"] = _check("running_var", rv, (1 - mom) * rv0 + mom * uv,
                                                     FORM * ((1 - mom) * rv0 + mom * uv) + mom * uv * (TOL_SUM + (mbar / sd) ** 2))
            else:       # documented divergence (nn.BatchNorm1d raises on one training row): variance 0, output beta
                assert torch.equal(_cpu(rv), _f32(_f32(1 - _f32(torch.tensor(mom, dtype=F64))) * rv0))
                assert torch.equal(_cpu(y)[0], beta.clamp_min(0) if relu else beta)
        else:
            assert torch.equal(smk, rm0)
            rs = 1 / torch.sqrt(rv0 + eps32)
            errs[f"{mode}_rstd"] = _check("eval rstd", srk, rs, rs * 4 * EPS32)
            assert torch.equal(_cpu(rm), rm0) and torch.equal(_cpu(rv), rv0), "eval mode changed the running statistics"
        xh = (x - smk) * srk
        yr = xh * gamma + beta
        if relu:
            yr = yr.clamp_min(0)
        errs[f"{mode}_y"] = _check(f"bn1d {mode} y", y, yr, FORM * ((xh * gamma).abs() + beta.abs()) + 1e-30)
        # backward from float64 statistics rounded to f32 (the reference uses the same f32 values); y read for the ReLU mask
        for frozen in ((False, True) if training else (True,)):
            dy = _rand((B, Fn), g)
            yk = _cpu(y)
            mu_b, rs_b = (smk, srk)
            dx, dgm, dbt = pkg.ops.bn1d_bwd(_dev32(dy), _dev32(x), y, _dev32(gamma), sm, sr, relu, frozen_stats=frozen)
            d = dy * (yk > 0) if relu else dy
            xhb = (x - mu_b) * rs_b
            sb, sg = d.sum(0), (d * xhb).sum(0)
            tb, tg = d.abs().sum(0), (d * xhb).abs().sum(0)
            tag = f"{mode}{'_frozen' if frozen else ''}"
            errs[f"{tag}_dbeta"] = _check("dbeta", dbt, sb, TOL_SUM * tb)
            errs[f"{tag}_dgamma"] = _check("dgamma", dgm, sg, TOL_SUM * tg + FORM * tg)
            if frozen:
                dxr = gamma * rs_b * d
                dxbar = FORM * (gamma * rs_b * d).abs()
            else:
                dxr = gamma * rs_b * (d - sb / B - xhb * sg / B)
                dxbar = (gamma * rs_b).abs() * (FORM * (d.abs() + (xhb * sg).abs() / B) + TOL_SUM * (tb + xhb.abs() * tg) / B)
            errs[f"{tag}_dx"] = _check(f"bn1d {tag} dx", dx, dxr, dxbar + 1e-30)
    _log(f"bn1d B{B} F{Fn}", errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. poolings and fusions (csrc/smallops.hip)
# ---------------------------------------------------------------------------------------------------------------------------------

def _launch(pkg, name, *args):
    _ok(pkg, getattr(_lib(pkg), name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _st()), name)


@pytest.mark.parametrize("S", [1, 5, 300])
def test_pool_max_mean(pkg, S):
    g = torch.Generator().manual_seed(900 + S)
    B, D = 5, 70
    h = _ints((B, S, D), g, -2, 2)            # ties everywhere: the first maximum must win
    if S > 1:
        h[1, 2 % S, 3] = float("nan")         # NaN propagates as in torch.max (first NaN wins)
        h[1, S - 1, 3] = float("nan")
        h[2, S - 1, 4] = float("nan")
    hd = _dev32(h)
    out = torch.empty((B, D), dtype=F32, device="cuda")
    arg = torch.empty((B, D), dtype=I32, device="cuda")
    _launch(pkg, "mh_pool_max_fwd", hd, out, arg, B, S, D)
    ref_v, ref_i = torch.max(h, dim=1)
    assert torch.equal(_cpu(out).nan_to_num(7.5), ref_v.nan_to_num(7.5)), "max"
    # first maximum / first NaN (torch.max's index for ties and NaN on CPU is not specified: compute it)
    first = torch.where(torch.isnan(h).any(1), torch.isnan(h).to(I64).argmax(1), (h == ref_v[:, None]).to(I64).argmax(1))
    assert torch.equal(arg.cpu().to(I64), first), "arg: not the first maximum / first NaN"
    dout = _rand((B, D), g)
    dh = torch.full((B, S, D), SENT32, dtype=F32, device="cuda")
    _launch(pkg, "mh_pool_max_bwd", _dev32(dout), arg, dh, B, S, D)
    want = torch.zeros(B, S, D, dtype=F64).scatter_(1, first[:, None], dout[:, None])
    assert torch.equal(_cpu(dh), want)
    # masked mean, one all-zero mask row
    hm = _rand((B, S, D), g)
    mask = (torch.rand(B, S, generator=g) < 0.6).to(I64)
    mask[0] = 0
    mask[1, 0] = 1
    out = torch.empty((B, D), dtype=F32, device="cuda")
    _launch(pkg, "mh_pool_mean_fwd", _dev32(hm), mask.cuda(), out, B, S, D)
    m = mask.to(F64)
    cnt = m.sum(1).clamp_min(1e-9)[:, None]
    e1 = _check("mean fwd", out, (hm * m[:, :, None]).sum(1) / cnt, TOL_SUM * (hm.abs() * m[:, :, None]).sum(1) / cnt)
    assert bool((_cpu(out)[0] == 0).all())
    dh = torch.empty((B, S, D), dtype=F32, device="cuda")
    _launch(pkg, "mh_pool_mean_bwd", _dev32(dout), mask.cuda(), dh, B, S, D)
    wr = dout[:, None, :] * m[:, :, None] / cnt[:, :, None]
    e2 = _check("mean bwd", dh, wr, 4 * EPS32 * wr.abs())
    _log(f"pool_max_mean S{S}", {"max": "bit-exact", "mean_fwd": e1, "mean_bwd": e2})


ATTN_CASES = [(s, a) for s in (1, 255, 256, 257, 1024) for a in (64, 300)]


@pytest.mark.parametrize("S,A", ATTN_CASES, ids=[f"S{s}_A{a}" for s, a in ATTN_CASES])
def test_pool_attn(pkg, S, A):
    g = torch.Generator().manual_seed(1000 + S + A)
    B, D = 3, 200
    h = _rand((B, S, D), g)
    u = _f32(torch.tanh(_rand((B, S, A), g, 2.0)))
    w2, b2 = _rand((A,), g, 1.0 / math.sqrt(A)), _rand((1,), g, 0.1)
    mask = (torch.rand(B, S, generator=g) < 0.7).to(I64)
    mask[0, 0] = 1
    mask[2] = 0                               # a fully masked row: uniform weights
    p = torch.empty((B, S), dtype=F32, device="cuda")
    out = torch.empty((B, D), dtype=F32, device="cuda")
    hd, ud, w2d = _dev32(h), _dev32(u), _dev32(w2)
    _launch(pkg, "mh_pool_attn_fwd", hd, ud, w2d, _dev32(b2), mask.cuda(), p, out, B, S, D, A)
    s64 = u @ w2 + b2
    sbar = TOL_SUM * (u.abs() @ w2.abs() + b2.abs()) + EPS32 * s64.abs()
    sc = (s64.to(F32) + (1.0 - mask.to(F32)) * -1e9).to(F64)       # the reference class adds the mask term in f32
    pr = torch.softmax(sc, 1)
    pbar = 2 * pr * sbar.max(1, keepdim=True).values + pr * (TOL_SUM + TRANS)
    errs = {"p": _check("attn p", p, pr, pbar)}
    pk = _cpu(p)
    assert torch.allclose(pk[2], torch.full((S,), 1.0 / S, dtype=F64), rtol=8 * EPS32 * (1 + S / 256), atol=0), "masked row"
    errs["out"] = _check("attn out", out, (pk[:, :, None] * h).sum(1), TOL_SUM * (pk[:, :, None] * h.abs()).sum(1))
    # backward from the kernel's own p
    dout = _rand((B, D), g)
    du = torch.empty((B, S, A), dtype=F32, device="cuda")
    dh = torch.empty((B, S, D), dtype=F32, device="cuda")
    dw2p = torch.empty((B, A), dtype=F32, device="cuda")
    db2p = torch.empty((B,), dtype=F32, device="cuda")
    _launch(pkg, "mh_pool_attn_bwd", hd, ud, w2d, p, _dev32(dout), du, dh, dw2p, db2p, B, S, D, A)
    dp = (h * dout[:, None, :]).sum(2)
    tdp = (h.abs() * dout.abs()[:, None, :]).sum(2)
    t = (pk * dp).sum(1, keepdim=True)
    ds = pk * (dp - t)
    tds = pk * (tdp + (pk * tdp).sum(1, keepdim=True))
    dsb = TOL_SUM * tds
    errs["du"] = _check("attn du", du, ds[:, :, None] * w2 * (1 - u * u),
                        (dsb + FORM * ds.abs())[:, :, None] * (w2.abs() * (1 + u * u)))
    errs["dw2_part"] = _check("attn dw2", dw2p, (ds[:, :, None] * u).sum(1), TOL_SUM * (tds[:, :, None] * u.abs()).sum(1))
    errs["db2_part"] = _check("attn db2", db2p, ds.sum(1), TOL_SUM * tds.sum(1))
    errs["dh"] = _check("attn dh", dh, pk[:, :, None] * dout[:, None, :], 2 * EPS32 * (pk[:, :, None] * dout[:, None, :]).abs())
    _log(f"pool_attn S{S} A{A}", errs)


@pytest.mark.parametrize("taps", [1, 3, 5, 7])
def test_conv_pool_pieces(pkg, taps):
    g = torch.Generator().manual_seed(1100 + taps)
    B, D = 3, 66
    for S in (2, 9):           # S < taps for taps 3 / 5 / 7 at S = 2
        pad = taps // 2
        Sp = S + 2 * pad
        h = _rand((B, S, D), g)
        hp = torch.full((B * Sp + 1, D), SENT32, dtype=F32, device="cuda")
        _launch(pkg, "mh_pad_seq_f32", _dev32(h), hp, B, S, D, pad, Sp)
        want = torch.zeros(B, Sp, D, dtype=F64)
        want[:, pad:pad + S] = h
        hpc = _cpu(hp)
        assert torch.equal(hpc[:B * Sp].view(B, Sp, D), want) and bool((hpc[B * Sp:] == SENT32).all()), "pad_seq"
        rows = B * Sp - (taps - 1)
        # relu_max: integers (ties, exact max), one column all <= 0 (arg -1)
        z = _ints((rows, D), g, -3, 3)
        z[:, 5] = -1.0
        out = torch.empty((B, D), dtype=F32, device="cuda")
        arg = torch.empty((B, D), dtype=I32, device="cuda")
        _launch(pkg, "mh_relu_max_fwd", _dev32(z), out, arg, B, S, Sp, D)
        win = torch.stack([z[b * Sp:b * Sp + S] for b in range(B)]).clamp_min(0)
        mx = win.max(1).values
        first = torch.where(mx > 0, (win == mx[:, None]).to(I64).argmax(1), torch.full_like(mx, -1).to(I64))
        assert torch.equal(_cpu(out), mx) and torch.equal(arg.cpu().to(I64), first), "relu_max fwd"
        dout = _rand((B, D), g)
        dz = torch.full((rows, D), SENT32, dtype=F32, device="cuda")
        _launch(pkg, "mh_relu_max_bwd", _dev32(dout), arg, dz, rows, Sp, D)
        wz = torch.zeros(rows, D, dtype=F64)
        for b in range(B):
            for o in range(D):
                if first[b, o] >= 0:
                    wz[b * Sp + first[b, o], o] = dout[b, o]
        assert torch.equal(_cpu(dz), wz), "relu_max bwd"
        # conv_fold on integers: exact
        da = _ints((rows, taps * D), g, -5, 5)
        dh = torch.empty((B, S, D), dtype=F32, device="cuda")
        _launch(pkg, "mh_conv_fold_f32", _dev32(da), dh, B, S, D, taps, pad, Sp, rows)
        wf = torch.zeros(B, S, D, dtype=F64)
        for b in range(B):
            for s in range(S):
                for j in range(taps):
                    w = s + pad - j
                    if 0 <= w < S and b * Sp + w < rows:
                        wf[b, s] += da[b * Sp + w, j * D:(j + 1) * D]
        assert torch.equal(_cpu(dh), wf), f"conv_fold taps {taps} S {S}"
    _log(f"conv_pool_pieces taps{taps}", {"pad_seq / relu_max / conv_fold": "bit-exact (S 2 and 9)"})


GATE_FS = [1, 63, 64, 65, 1536]


@pytest.mark.parametrize("Fn", GATE_FS)
def test_softmax_gate(pkg, Fn):
    g = torch.Generator().manual_seed(1200 + Fn)
    B = 9
    errs = {}
    for off in (0.0, 1e4):
        gi = _rand((B, Fn), g, 3.0, off)
        c, dy = _rand((B, Fn), g), _rand((B, Fn), g)
        y = torch.empty((B, Fn), dtype=F32, device="cuda")
        gd, cd = _dev32(gi), _dev32(c)
        _launch(pkg, "mh_softmax_gate_fwd", gd, cd, y, B, Fn)
        p = torch.softmax(gi, 1)
        pb = p * (TOL_SUM + TRANS)      # g - max is exact (Sterbenz) even at 1e4; expf and the normaliser's f32 sum
        errs[f"y_off{off:g}"] = _check("gate y", y, p * c, pb * c.abs())
        dg = torch.empty_like(y)
        dc = torch.empty_like(y)
        _launch(pkg, "mh_softmax_gate_bwd", gd, cd, _dev32(dy), dg, dc, B, Fn)
        errs[f"dc_off{off:g}"] = _check("gate dc", dc, p * dy, pb * dy.abs() + EPS32 * (p * dy).abs())
        t = (p * dy * c).sum(1, keepdim=True)
        tt = (p * (dy * c).abs()).sum(1, keepdim=True)
        errs[f"dg_off{off:g}"] = _check("gate dg", dg, p * (dy * c - t), pb * ((dy * c).abs() + tt) + p * TOL_SUM * tt)
    _log(f"softmax_gate F{Fn}", errs)


MCA_BS = [1, 2, 255, 256, 257, 1024]


def _mca_ref_e(pa, pc, pi, V, bv):
    """float64 e[i][j] = V . tanh(pa[j] + pc[j] + pi[i]) + bv and its bar terms, chunked over i"""
    B, U = pa.shape
    e = torch.empty(B, B, dtype=F64)
    te = torch.empty(B, B, dtype=F64)
    base = pa + pc
    for i0 in range(0, B, 64):
        arg = base[None, :, :] + pi[i0:i0 + 64, None, :]
        th = torch.tanh(arg)
        e[i0:i0 + 64] = th @ V + bv
        te[i0:i0 + 64] = (1 + arg.abs()) @ V.abs()
    return e, TOL_SUM * te + TRANS * V.abs().sum()


@pytest.mark.parametrize("B", MCA_BS)
def test_mca3(pkg, B):
    g = torch.Generator().manual_seed(1300 + B)
    U = 72
    pa, pc, pi = (_rand((B, U), g, 0.5) for _ in range(3))
    V, bv = _rand((U,), g, 1.0 / math.sqrt(U)), _rand((1,), g, 0.1)
    text, cap = _rand((B, U), g), _rand((B, U), g)
    dv = [_dev32(t) for t in (pa, pc, pi, V, bv, text, cap)]
    w = torch.empty((B, B), dtype=F32, device="cuda")
    ctx = torch.empty((B, 2 * U), dtype=F32, device="cuda")
    _launch(pkg, "mh_mca3_fwd", *dv, w, ctx, B, U)
    e, ebar = _mca_ref_e(pa, pc, pi, V, bv)
    wr = torch.softmax(e, 1)
    errs = {"w": _check("mca3 w", w, wr, 2 * wr * ebar.max(1, keepdim=True).values + wr * (TOL_SUM + TRANS))}
    wk = _cpu(w)
    ref_ctx = torch.cat([wk @ text, wk @ cap], 1)
    errs["ctx"] = _check("mca3 ctx", ctx, ref_ctx, TOL_SUM * torch.cat([wk @ text.abs(), wk @ cap.abs()], 1))
    # backward from the kernel's own w and de
    dctx = _rand((B, 2 * U), g)
    de, dpa, dpi, dt, dc, dVp = (torch.empty(s, dtype=F32, device="cuda") for s in ((B, B), (B, U), (B, U), (B, U), (B, U), (B, U)))
    dbp = torch.empty((B,), dtype=F32, device="cuda")
    _launch(pkg, "mh_mca3_bwd", dv[0], dv[1], dv[2], dv[3], dv[5], dv[6], w, _dev32(dctx), de, dpa, dpi, dt, dc, dVp, dbp, B, U)
    d1, d2 = dctx[:, :U], dctx[:, U:]
    d = d1 @ text.t() + d2 @ cap.t()
    td = d1.abs() @ text.abs().t() + d2.abs() @ cap.abs().t()
    t = (wk * d).sum(1, keepdim=True)
    errs["de"] = _check("mca3 de", de, wk * (d - t), TOL_SUM * wk * (td + (wk * td).sum(1, keepdim=True)) + FORM * (wk * (d - t)).abs())
    dek = _cpu(de)
    base = pa + pc
    gp_i = torch.empty(B, U, dtype=F64)
    gv_i = torch.empty(B, U, dtype=F64)
    tg_i = torch.empty(B, U, dtype=F64)
    gp_j = torch.zeros(B, U, dtype=F64)
    tg_j = torch.zeros(B, U, dtype=F64)
    for i0 in range(0, B, 64):
        arg = base[None, :, :] + pi[i0:i0 + 64, None, :]          # [i][j][k]
        th = torch.tanh(arg)
        dd = dek[i0:i0 + 64, :, None]
        sech = 1 - th * th
        gp_i[i0:i0 + 64] = (dd * sech).sum(1)
        gv_i[i0:i0 + 64] = (dd * th).sum(1)
        tg_i[i0:i0 + 64] = (dd.abs() * (1 + arg.abs())).sum(1)
        gp_j += (dd * sech).sum(0)
        tg_j += (dd.abs() * (1 + arg.abs())).sum(0)
    errs["dpi"] = _check("mca3 dpi", dpi, gp_i * V, (TOL_SUM + TRANS) * tg_i * V.abs())
    errs["dV_part"] = _check("mca3 dV_part", dVp, gv_i, (TOL_SUM + TRANS) * tg_i)
    errs["dbv_part"] = _check("mca3 dbv_part", dbp, dek.sum(1), TOL_SUM * dek.abs().sum(1))
    errs["dpa"] = _check("mca3 dpa", dpa, gp_j * V, (TOL_SUM + TRANS) * tg_j * V.abs())
    errs["dtext"] = _check("mca3 dtext", dt, wk.t() @ d1, TOL_SUM * (wk.t() @ d1.abs()))
    errs["dcap"] = _check("mca3 dcap", dc, wk.t() @ d2, TOL_SUM * (wk.t() @ d2.abs()))
    _log(f"mca3 B{B} U{U}", errs)


def _grads64(fn, inputs):
    xs = [x.clone().requires_grad_(True) for x in inputs]
    out = fn(*xs)
    return out, xs


def _grads_dev(fn, inputs, dout):
    xs = [_dev32(x).requires_grad_(True) for x in inputs]
    out = fn(*xs)
    out.backward(_dev32(dout))
    return out, xs


# inputs whose gradient is exactly 0 by an invariance of the formula (softmax over s / j is shift invariant: d b2 = d bv = 0;
# BatchNorm removes a per-column constant: d bias of the Linear under it = 0): the kernel's value is rounding noise of a sum, held to
# COMP x sum|terms| -- the float64 sum of |the gradient of the intermediate the bias is added to|
_AUX = {}
ZERO_GRADS = {"attention_pool": (4, "s"), "attention_pool_masked_row": (4, "s"), "mca3_B257": (4, "e"), "linear_bn_relu_B40": (2, "z"),
              "linear_bn_relu_B100": (2, "z")}


def _keep(name, t):
    t.retain_grad()
    _AUX[name] = t
    return t


FUSED_OPS = ["max_pool", "mean_pool", "attention_pool", "attention_pool_masked_row", "conv_pool_k3", "conv_pool_k7_S2",
             "conv_pool_nonpositive", "softmax_gate", "mca3_B257", "linear_tanh", "linear_bn_relu_B40", "linear_bn_relu_B100"]


@pytest.mark.parametrize("op", FUSED_OPS)
def test_fused_autograd(pkg, op):
    """fused.py's autograd Functions (kernel + GEMM + colsum chains) against float64 autograd of the reference formula"""
    fz = pkg.fused
    g = torch.Generator().manual_seed(1400 + FUSED_OPS.index(op))
    B, S, D = 4, 37, 72
    if op in ("max_pool", "mean_pool") or op.startswith("attention_pool"):
        h = _rand((B, S, D), g)
        mask = (torch.rand(B, S, generator=g) < 0.7).to(I64)
        mask[:, 0] = 1
        if op == "attention_pool_masked_row":
            mask[1] = 0
        A = 300
        W1, b1 = _rand((A, D), g, 1 / math.sqrt(D)), _rand((A,), g, 0.1)
        w2, b2 = _rand((1, A), g, 1 / math.sqrt(A)), _rand((1,), g, 0.1)
        if op == "max_pool":
            fdev = lambda hh: fz.max_pool(hh)
            f64 = lambda hh: torch.max(hh, 1).values
            ins = [h]
        elif op == "mean_pool":
            md = mask.cuda()
            fdev = lambda hh: fz.masked_mean_pool(hh, md)
            m = mask.to(F64)
            f64 = lambda hh: (hh * m[:, :, None]).sum(1) / m.sum(1, keepdim=True).clamp_min(1e-9)
            ins = [h]
        else:
            md = mask.cuda()
            fdev = lambda hh, a, b, c, d: fz.attention_pool(hh, md, a, b, c, d)
            mterm = (1.0 - mask.to(F32)) * -1e9

            def f64(hh, a, b, c, d):
                s = _keep("s", (torch.tanh(hh @ a.t() + b) @ c.t()).squeeze(-1) + d)
                s = s + ((s.detach().to(F32) + mterm).to(F64) - s.detach())       # the f32 addition of the masked term
                return (torch.softmax(s, 1)[:, :, None] * hh).sum(1)
            ins = [h, W1, b1, w2, b2]
    elif op.startswith("conv_pool"):
        taps, S2 = {"conv_pool_k3": (3, S), "conv_pool_k7_S2": (7, 2), "conv_pool_nonpositive": (5, 6)}[op]
        h = _rand((B, S2, D), g)
        W, bb = _rand((D, D, taps), g, 1 / math.sqrt(D * taps)), _rand((D,), g, 0.1)
        if op == "conv_pool_nonpositive":        # every pre-activation <= 0: output 0, arg -1, all gradients 0
            h, W, bb = h.abs(), -W.abs(), -bb.abs() - 0.1
        fdev = lambda hh, ww, b_: fz.conv1d_relu_max_pool(hh, ww, b_)
        f64 = lambda hh, ww, b_: torch.relu(torch.nn.functional.conv1d(hh.transpose(1, 2), ww, b_, padding=taps // 2)).max(2).values
        ins = [h, W, bb]
    elif op == "softmax_gate":
        gi, c = _rand((B, 1536), g, 3.0), _rand((B, 1536), g)
        fdev = lambda a, b: fz.softmax_gate(a, b)
        f64 = lambda a, b: torch.softmax(a, 1) * b
        ins = [gi, c]
    elif op == "mca3_B257":
        Bm, U = 257, 72
        ins = [_rand((Bm, U), g, 0.5) for _ in range(3)] + [_rand((1, U), g, 1 / math.sqrt(U)), _rand((1,), g, 0.1),
                                                            _rand((Bm, U), g), _rand((Bm, U), g)]
        fdev = lambda *a: fz.mca3_attention(*a)

        def f64(pa, pc, pi, V, bv, t, cp):
            e = _keep("e", torch.tanh(pa[None, :, :] + pc[None, :, :] + pi[:, None, :]) @ V.view(-1) + bv)
            w = torch.softmax(e, 1)
            return torch.cat([w @ t, w @ cp], 1)
    elif op == "linear_tanh":
        x, W, b = _rand((70, 130), g), _rand((65, 130), g, 1 / math.sqrt(130)), _rand((65,), g, 0.3)
        fdev = lambda a, b_, c: fz.linear(a, b_, c, act="tanh")
        f64 = lambda a, b_, c: torch.tanh(a @ b_.t() + c)
        ins = [x, W, b]
    else:
        Bn = 40 if op.endswith("B40") else 100       # one fused launch (M <= 64) / the GEMM + mh_bn1d path
        x, W, b = _rand((Bn, 96), g), _rand((65, 96), g, 1 / math.sqrt(96)), _rand((65,), g, 0.3)
        gm, bt = _rand((65,), g, 0.3, 1.0), _rand((65,), g, 0.3)
        lin, bn = torch.nn.Linear(96, 65).cuda(), torch.nn.BatchNorm1d(65).cuda().train()

        def f64(a, w_, b_, gg, bb):
            z = _keep("z", a @ w_.t() + b_)
            return torch.relu(torch.nn.functional.batch_norm(z, None, None, gg, bb, training=True, eps=1e-5))
        ins = [x, W, b, gm, bt]
    out64, xs64 = _grads64(f64, ins)
    dout = _rand(tuple(out64.shape), g)
    out64.backward(dout)
    if op.startswith("linear_bn"):
        xs = [_dev32(t).requires_grad_(True) for t in ins]
        lin.weight, lin.bias = torch.nn.Parameter(xs[1].detach().clone()), torch.nn.Parameter(xs[2].detach().clone())
        bn.weight, bn.bias = torch.nn.Parameter(xs[3].detach().clone()), torch.nn.Parameter(xs[4].detach().clone())
        out = fz.linear_bn_act(xs[0], lin, bn, relu=True)
        out.backward(_dev32(dout))
        got_grads = [xs[0].grad, lin.weight.grad, lin.bias.grad, bn.weight.grad, bn.bias.grad]
    else:
        out, xs = _grads_dev(fdev, ins, dout)
        got_grads = [x.grad for x in xs]
    errs = {"out": _comp(f"{op} out", out, out64.detach())}
    for k, (gg, x64) in enumerate(zip(got_grads, xs64)):
        assert gg is not None, f"{op}: no gradient for input {k}"
        if ZERO_GRADS.get(op, (None,))[0] == k:
            ga = _AUX[ZERO_GRADS[op][1]].grad.abs()
            terms = float(ga.sum() if x64.numel() == 1 else ga.sum(0).max())      # a scalar bias sums every element
            errs[f"d{k}_zero_by_invariance"] = _check(f"{op} d{k} (0 by invariance)", gg, x64.grad, COMP * terms)
        else:
            errs[f"d{k}"] = _comp(f"{op} d{k}", gg, x64.grad)
    if op == "conv_pool_nonpositive":
        assert bool((_cpu(out) == 0).all()) and all(bool((_cpu(gg) == 0).all()) for gg in got_grads)
    _log(f"fused_autograd {op}", errs)


@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5])
def test_colsum(pkg, rows):
    g = torch.Generator().manual_seed(1500 + rows)
    worst = 0.0
    for D in (1, 63, 64, 65):
        ld = D + 3
        x = _rand((rows, ld), g)
        x[:, D:] = float("nan")                 # columns [D, ld) must not be read
        out = torch.full((D + 2,), SENT32, dtype=F32, device="cuda")
        scale = 0.3
        xd = _dev32(x)
        _ok(pkg, _lib(pkg).mh_colsum_f32(xd.data_ptr(), ld, out.data_ptr(), rows, D, scale, _st()), "mh_colsum_f32")
        oc = _cpu(out)
        assert bool((oc[D:] == SENT32).all())
        xs = x[:, :D]
        s32 = float(np.float32(scale))
        worst = max(worst, _check(f"colsum rows{rows} D{D}", oc[:D], s32 * xs.sum(0), s32 * (TOL_SUM * xs.abs().sum(0))
                                  + EPS32 * (s32 * xs.sum(0)).abs()))
        xi = _ints((rows, ld), g, -9, 9)       # integers: exact sums, one f32 multiply by scale
        xid = _dev32(xi)
        _ok(pkg, _lib(pkg).mh_colsum_f32(xid.data_ptr(), ld, out.data_ptr(), rows, D, scale, _st()), "mh_colsum_f32")
        assert torch.equal(_cpu(out)[:D], _f32(s32 * xi[:, :D].sum(0)))
    _log(f"colsum rows{rows}", {"out": worst, "int": "bit-exact"})


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. optimizer and wire (csrc/optim.hip)
# ---------------------------------------------------------------------------------------------------------------------------------

SUMSQ_NS = [1, 2, 3, 4, 5, 4 * 1237 + 3, 300_001, (1 << 25) + 3]


@pytest.mark.parametrize("n", SUMSQ_NS)
def test_sumsq(pkg, n):
    g = torch.Generator().manual_seed(1600)
    x = _rand((n,), g, 2.0)
    x[-1] = 3.0                           # the n % 4 tail is not negligible
    ws = torch.full((1024,), SENT32, dtype=F32, device="cuda")
    out = torch.empty(1, dtype=F32, device="cuda")
    pkg.ops.sumsq(_dev32(x), ws, out)
    ref = (x * x).sum()
    e = _check(f"sumsq n{n}", out, ref.reshape(1), TOL_SUM * ref)
    nb = min(max(1, min((n // 32 + 1 + 255) // 256, 2048)), 1024)
    _log(f"sumsq n{n}", {"sum": e, "partials": nb})


HYPER_DEFAULT = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, t=1, gs=1.0)


def _hyper(lr, b1, b2, eps, wd, t, gs):
    return torch.tensor([lr, b1, b2, eps, wd, 1 / (1 - b1 ** t), 1 / math.sqrt(1 - b2 ** t), gs], dtype=F32)


def _adam_ref(p, m, v, g, h, decoupled, gnorm=None, max_norm=0.0, cm=0.0):
    """float64 Adam from the f32 inputs and f32 hyper h (float64 tensor of 8); returns (p, m, v, bars) or None (skipped step)"""
    lr, b1, b2, eps, wd, ibc1, isbc2, gs = (float(x) for x in h)
    cbar = 0.0
    if gnorm is not None:
        nrm = math.sqrt(gnorm) * abs(gs)
        if not nrm <= 3.0e38:
            return None
        nc = math.sqrt(gnorm) * cm if cm > 0 else nrm
        if max_norm > 0:
            gs *= min(1.0, max_norm / (nc + 1e-6))
            cbar = 8 * EPS32
    step = lr * ibc1
    decay = 1 - lr * wd if decoupled else 1.0
    l2 = 0.0 if decoupled else wd
    w = p * decay
    gg = g * gs + l2 * w
    mm = m * b1 + (1 - b1) * gg
    v2 = v * b2 + (1 - b2) * gg * gg
    upd = step * mm / (torch.sqrt(v2) * isbc2 + eps)
    pn = w - upd
    bars = (FORM * (w.abs() + upd.abs()) + cbar * upd.abs(),
            FORM * ((m * b1).abs() + ((1 - b1) * gg).abs()) + cbar * ((1 - b1) * gg).abs(),
            FORM * ((v * b2).abs() + (1 - b2) * gg * gg) + 2 * cbar * (1 - b2) * gg * gg)
    return pn, mm, v2, bars


ADAM_CASES = {    # name: (n, n_shadow, decoupled, wd, gs, max_norm, clip_norm_mult, gnorm_kind)
    "n4_adam": (4, 4, False, 0.0, 1.0, 0.0, 0.0, None),
    "n8_l2_shadow0": (8, 0, False, 0.01, 1.0, 0.0, 0.0, None),
    "n4948_adamw_shadow_part": (4948, 2000, True, 0.01, 1.0, 0.0, 0.0, None),
    "n4948_l2_gs_neg": (4948, 4948, False, 0.05, -0.5, 0.0, 0.0, None),
    "n4948_clip": (4948, 4948, True, 0.01, 0.25, 1.0, 0.0, "f"),
    "n4948_clip_mult": (4948, 4948, False, 0.0, 1.0 / 1024, 1.0, 1024.0, "f"),
    "n4948_clip_inactive": (4948, 4948, True, 0.01, 1.0, 1e6, 0.0, "f"),
    "n4194348_two_trips": (4_194_348, 4_194_000, True, 0.01, 2.0, 1.0, 0.0, "f"),
    "n4948_norm_inf": (4948, 4948, True, 0.01, 1.0, 1.0, 0.0, "inf"),
    "n4948_norm_nan": (4948, 4948, False, 0.0, 1.0, 0.0, 0.0, "nan"),
}


@DTYPES
@pytest.mark.parametrize("case", list(ADAM_CASES))
def test_adam(pkg, case, T16):
    n, ns, dec, wd, gs, mx, cm, gk = ADAM_CASES[case]
    g = torch.Generator().manual_seed(1700 + list(ADAM_CASES).index(case))
    p, gr = _rand((n,), g), _rand((n,), g, 3.0)
    m, v = _rand((n,), g, 0.1), _f32(torch.rand(n, generator=g, dtype=F64) * 0.01)
    h = _hyper(1e-3, 0.9, 0.999, 1e-8, wd, 3, gs)
    gnorm = None
    if gk == "f":
        gnorm = float(np.float32((gr * gr).sum()))
    elif gk == "inf":
        gnorm = float("inf")
    elif gk == "nan":
        gnorm = float("nan")
    pd, md, vd = _dev32(p), _dev32(m), _dev32(v)
    shadow = _sent16(n + 8, T16)
    gn = None if gnorm is None else torch.tensor([gnorm], dtype=F32, device="cuda")
    pkg.ops.adam_step(pd, md, vd, _dev32(gr), shadow, ns, h.cuda(), decoupled=dec, gnorm_sq=gn, max_norm=mx, clip_norm_mult=cm)
    torch.cuda.synchronize()
    r = _adam_ref(p, m, v, gr, h.to(F64), dec, gnorm, mx, cm)
    sh = shadow.cpu()
    if r is None:       # non-finite norm: nothing moves, bit for bit
        assert _same_bits(pd, p.to(F32)) and _same_bits(md, m.to(F32)) and _same_bits(vd, v.to(F32)), "skipped step moved state"
        assert bool((sh.view(I16) == SENT16).all()), "skipped step wrote the shadow"
        _log(f"adam {case} {_name(T16)}", {"p,m,v,shadow": "untouched bit for bit"})
        return
    pn, mn, vn, (bp, bm, bv) = r
    errs = {"p": _check(f"adam {case} p", pd, pn, bp), "m": _check("m", md, mn, bm), "v": _check("v", vd, vn, bv)}
    assert _same_bits(sh[:ns], pd.cpu()[:ns].to(T16)), "shadow != p.to(T16)"
    assert bool((sh[ns:].view(I16) == SENT16).all()), "shadow words past n_shadow written"
    _log(f"adam {case} {_name(T16)}", errs)


def test_adam_state_carried(pkg):
    """five steps, state carried on both sides, against a float64 Adam (L2) and AdamW"""
    n = 4 * 5003
    errs = {}
    for dec in (False, True):
        g = torch.Generator().manual_seed(1800 + dec)
        p = _rand((n,), g)
        p64, m64, v64 = p.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
        pd, md, vd = _dev32(p), torch.zeros(n, dtype=F32, device="cuda"), torch.zeros(n, dtype=F32, device="cuda")
        acc = [torch.zeros(n, dtype=F64) for _ in range(3)]
        for t in range(1, 6):
            gr = _rand((n,), g, 0.0 if t == 3 else 1.0)
            h = _hyper(1e-3, 0.9, 0.999, 1e-8, 0.01, t, 1.0)
            pkg.ops.adam_step(pd, md, vd, _dev32(gr), None, 0, h.cuda(), decoupled=dec)
            p64, m64, v64, bars = _adam_ref(p64, m64, v64, gr, h.to(F64), dec)
            for a, b in zip(acc, bars):
                a += b
        tag = "adamw" if dec else "adam_l2"
        # errors add up over the steps (each step's bar), and one step's error in m / v moves later updates by less than it: 2x
        errs[f"{tag}_p"] = _check("carried p", pd, p64, 2 * acc[0])
        errs[f"{tag}_m"] = _check("carried m", md, m64, 2 * acc[1])
        errs[f"{tag}_v"] = _check("carried v", vd, v64, 2 * acc[2])
    _log("adam_state_carried 5 steps", errs)


@DTYPES
def test_adam_guarded(pkg, T16):
    n = 4 * 70_000
    g = torch.Generator().manual_seed(1900)
    p, gr = _rand((n,), g), _rand((n,), g)
    m, v = _rand((n,), g, 0.1), _f32(torch.rand(n, generator=g, dtype=F64) * 0.01)
    bad_chunks = [1, 17, 40_000, n // 4 - 1]
    gb = gr.clone()
    for k, c in enumerate(bad_chunks):
        gb[4 * c + (k % 4)] = [float("inf"), float("nan"), -float("inf"), float("nan")][k]
    h = _hyper(1e-3, 0.9, 0.999, 1e-8, 0.01, 2, 1.0).cuda()

    def run(grad, mark, ordinal, guarded=True):
        st = [_dev32(x) for x in (p, m, v)]
        sh = _sent16(n, T16)
        ov = torch.tensor([mark], dtype=I32, device="cuda") if guarded else None
        pkg.ops.adam_step(*st, _dev32(grad), sh, n, h, decoupled=True, overflow=ov, ordinal=ordinal)
        torch.cuda.synchronize()
        return [x.cpu() for x in st] + [sh.cpu()], (int(ov) if guarded else None)

    plain, _ = run(gr, 0, 0, guarded=False)
    # 1. an EARLIER launch's mark: the whole launch is a no-op, the mark stays
    out, mark = run(gb, 2, 3)
    assert mark == 2
    assert all(_same_bits(a, b.to(F32)) for a, b in zip(out[:3], (p, m, v))) and bool((out[3].view(I16) == SENT16).all())
    # 2. its own mark (or a later one) does not stop it: with finite gradients == the unguarded launch bit for bit
    for pre in (3, 5):
        out, mark = run(gr, pre, 3)
        assert mark == pre and all(_same_bits(a, b) for a, b in zip(out, plain)), f"mark {pre} changed a finite launch"
    # 3. no mark yet, non-finite gradients: exactly the 4-element vectors holding one keep p, m, v (and shadow); every other
    #    vector -- also those after the first bad one, in other workgroups -- is updated == the unguarded launch bit for bit
    out, mark = run(gb, 0, 3)
    assert mark == 3, "the launch did not mark *overflow with its ordinal"
    badv = torch.zeros(n // 4, dtype=torch.bool)
    badv[bad_chunks] = True
    bad = badv.repeat_interleave(4)
    for k, (a, orig, pl) in enumerate(zip(out[:3], (p, m, v), plain[:3])):
        assert _same_bits(a[bad], orig[bad].to(F32)), f"state {k}: a vector with a non-finite gradient moved"
        assert _same_bits(a[~bad], pl[~bad]), f"state {k}: a finite vector differs from the unguarded update"
    assert bool((out[3][bad].view(I16) == SENT16).all()) and _same_bits(out[3][~bad], plain[3][~bad])
    _log(f"adam_guarded {_name(T16)}", {"rule": "earlier mark = no-op; own mark skips exactly the 4-element vectors with a "
                                                "non-finite gradient; bit-exact"})


ROWS_CASES = [(d, r) for d in (4, 8, 260, 768) for r in (1, 5)] + [(4, 30522), (768, 30522)]


@pytest.mark.parametrize("D,rows", ROWS_CASES, ids=[f"D{d}_rows{r}" for d, r in ROWS_CASES])
def test_adam_rows(pkg, D, rows):
    g = torch.Generator().manual_seed(2000 + D + rows)
    n = rows * D
    p, gr = _rand((n,), g), _rand((n,), g)
    m, v = _rand((n,), g, 0.1), _f32(torch.rand(n, generator=g, dtype=F64) * 0.01)
    live0 = (torch.rand(rows, generator=g) < 0.3).to(U8)
    touched = (torch.rand(rows, generator=g) < 0.3).to(U8)
    if rows > 1:
        live0[0], touched[0] = 0, 0          # one dead row at least
        live0[-1], touched[-1] = 0, 1
    h = _hyper(1e-3, 0.9, 0.999, 1e-8, 0.01, 4, 0.5)
    errs = {}
    for tnull in (False, True):
        st = [_dev32(x) for x in (p, m, v)]
        live = live0.cuda()
        pkg.ops.adam_step_rows(*st, _dev32(gr), live, None if tnull else touched.cuda(), rows, D, h.cuda(), decoupled=False)
        torch.cuda.synchronize()
        want_live = live0.clone() if tnull else (live0 | touched)
        assert torch.equal(live.cpu(), want_live), "row_live"
        lr_ = want_live.bool().repeat_interleave(D)
        for k, (a, orig) in enumerate(zip(st, (p, m, v))):
            assert _same_bits(a.cpu()[~lr_], orig[~lr_].to(F32)), f"state {k}: a dead row moved"
        if bool(lr_.any()):
            pn, mn, vn, (bp, bm, bv) = _adam_ref(p[lr_], m[lr_], v[lr_], gr[lr_], h.to(F64), False)
            tag = "tnull_" if tnull else ""
            errs[tag + "p"] = _check("rows p", st[0].cpu()[lr_], pn, bp)
            errs[tag + "m"] = _check("rows m", st[1].cpu()[lr_], mn, bm)
            errs[tag + "v"] = _check("rows v", st[2].cpu()[lr_], vn, bv)
    # all rows live == mh_adam_step on the same buffer, bit for bit (the same formula)
    st = [_dev32(x) for x in (p, m, v)]
    pkg.ops.adam_step_rows(*st, _dev32(gr), torch.ones(rows, dtype=U8, device="cuda"), None, rows, D, h.cuda())
    st2 = [_dev32(x) for x in (p, m, v)]
    pkg.ops.adam_step(*st2, _dev32(gr), None, 0, h.cuda())
    assert all(_same_bits(a, b) for a, b in zip(st, st2)), "all-live rows != the dense update"
    # guarded: an inf in row 0's first vector marks the ordinal and keeps that vector only
    if rows > 1:
        gb = gr.clone()
        gb[1] = float("inf")
        st = [_dev32(x) for x in (p, m, v)]
        ov = torch.zeros(1, dtype=I32, device="cuda")
        pkg.ops.adam_step_rows(*st, _dev32(gb), torch.ones(rows, dtype=U8, device="cuda"), None, rows, D, h.cuda(), overflow=ov, ordinal=2)
        torch.cuda.synchronize()
        assert int(ov) == 2
        for a, orig, b in zip(st, (p, m, v), st2):
            a = a.cpu()
            assert _same_bits(a[:4], orig[:4].to(F32)) and _same_bits(a[4:], b.cpu()[4:])
        ov.fill_(1)
        st = [_dev32(x) for x in (p, m, v)]
        pkg.ops.adam_step_rows(*st, _dev32(gr), torch.ones(rows, dtype=U8, device="cuda"), None, rows, D, h.cuda(), overflow=ov, ordinal=2)
        assert all(_same_bits(a, orig.to(F32)) for a, orig in zip(st, (p, m, v))), "an earlier mark did not stop the rows launch"
    errs["all_live==dense"] = "bit-exact"
    _log(f"adam_rows D{D} rows{rows}", errs)


SKIP_SCRIPT = [0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1] + [0] * 16 + [1, 0]      # 1 = the step overflowed


@pytest.mark.parametrize("groups,interval,use_norm", [(1, 1, True), (3, 3, False), (8, 1, False), (2, 3, True)])
def test_adam_skip_account(pkg, groups, interval, use_norm):
    L = _lib(pkg)
    b1s = [0.9 - 0.05 * k for k in range(groups)]
    b2s = [0.999 - 0.002 * k for k in range(groups)]
    hyp = [torch.zeros(8, dtype=F32, device="cuda") for _ in range(groups)]
    grp = pkg._lib.MhAdamSkipGroups()
    grp.n = groups
    for k in range(groups):
        grp.hyper[k] = hyp[k].data_ptr()
        grp.beta1[k], grp.beta2[k] = b1s[k], b2s[k]
    base = 0.25
    gf, bf, mn, mxs = 2.0, 0.5, 2.0 ** 12, 2.0 ** 16
    sc = torch.tensor([2.0 ** 15], dtype=F32, device="cuda")
    gr = torch.zeros(1, dtype=I32, device="cuda")
    ovf = torch.zeros(1, dtype=I32, device="cuda")
    ls = pkg._lib.MhLossScale()
    ls.scale, ls.growth, ls.overflow = sc.data_ptr(), gr.data_ptr(), ovf.data_ptr()
    ls.growth_factor, ls.backoff_factor, ls.min_scale, ls.max_scale = gf, bf, mn, mxs
    ls.growth_interval, ls.base_grad_scale = interval, base
    state = torch.zeros(2, dtype=I32, device="cuda")
    stepd = torch.zeros(1, dtype=I32, device="cuda")
    gn = torch.zeros(1, dtype=F32, device="cuda")
    # Python model: GradScaler.update in f32, t advancing only on clean steps
    m_sc, m_gr, skipped = np.float32(2.0 ** 15), 0, 0
    h7 = np.float32(1.0)
    hit_min = hit_max = False
    for step, bad in enumerate(SKIP_SCRIPT):
        for hh in hyp:
            hh[7] = float(h7)
        stepd.fill_(step)
        if use_norm:
            gn.fill_(float("inf") if bad else 3.0)
        else:
            ovf.fill_(2 if bad else 0)
        _ok(pkg, L.mh_adam_skip_account(C.byref(grp), gn.data_ptr() if use_norm else None, state.data_ptr(), stepd.data_ptr(),
                                        C.byref(ls), _st()), "mh_adam_skip_account")
        torch.cuda.synchronize()
        skipped += bad
        if bad:
            hit_min |= np.float32(m_sc * np.float32(bf)) < mn
            m_sc, m_gr = max(np.float32(m_sc * np.float32(bf)), np.float32(mn)), 0
        else:
            m_gr += 1
            if m_gr >= interval:
                hit_max |= np.float32(m_sc * np.float32(gf)) > mxs
                m_sc, m_gr = min(np.float32(m_sc * np.float32(gf)), np.float32(mxs)), 0
        t = max(step + 1 - skipped, 1)
        h7 = np.float32(base) * (np.float32(1.0) / m_sc)
        assert state.cpu().tolist() == [skipped, bad], (step, state.cpu().tolist())
        assert float(sc) == float(m_sc) and int(gr) == m_gr, (step, float(sc), float(m_sc), int(gr), m_gr)
        assert int(ovf) == 0, "overflow word not cleared"
        for k, hh in enumerate(hyp):
            hc = hh.cpu()
            w5 = np.float32(1.0 / (1.0 - b1s[k] ** t))
            w6 = np.float32(1.0 / math.sqrt(1.0 - b2s[k] ** t))
            assert (float(hc[5]), float(hc[6]), float(hc[7])) == (float(w5), float(w6), float(h7)), (step, k, hc.tolist())
    assert hit_min and hit_max, "the script must reach both clamps"
    _log(f"adam_skip_account groups{groups} interval{interval} {'gnorm' if use_norm else 'flag'}",
         {"state / scale / growth / hyper[5..7]": f"bit-exact over {len(SKIP_SCRIPT)} steps"})


def _special_f32(T16, g):
    fin = torch.finfo(T16)
    vals = [0.0, -0.0, 1.0, -1.0, float("inf"), -float("inf"), float("nan"), fin.max, -fin.max, fin.max * 1.01, fin.max * 2,
            fin.tiny, fin.tiny / 4, fin.tiny * 0.75, 1e-40, -1e-40, 1e-45, 3.4e38, -3.4e38, 65519.0, 65520.0, 65536.0]
    x = torch.tensor(vals, dtype=F32)
    # halfway points between neighbouring 16-bit values (RNE ties), both parities, and just either side of them
    base = (torch.randn(64, generator=g) * torch.pow(2.0, torch.randint(-12, 12, (64,), generator=g).float())).to(T16)
    nxt = (base.view(I16) + 1).view(T16)          # the next 16-bit value away from zero
    lo, hi = base.to(F32), nxt.to(F32)
    mid = ((lo.to(F64) + hi.to(F64)) / 2).to(F32)
    up = torch.nextafter(mid, torch.full_like(mid, float("inf")))
    dn = torch.nextafter(mid, torch.full_like(mid, -float("inf")))
    rnd = torch.randn(300, generator=g) * torch.pow(2.0, torch.randint(-30, 30, (300,), generator=g).float())
    return torch.cat([x, mid, up, dn, rnd]).to(F32)


@DTYPES
def test_casts(pkg, T16):
    g = torch.Generator().manual_seed(2100)
    special = _special_f32(T16, g)
    ns = list(range(1, 18)) + [8 * k + d for k in (3, 64, 1000) for d in (-1, 0, 1)] + [(1 << 20) + 5]
    nan_bits_same = True
    for n in ns:
        src = special[torch.arange(n) % special.numel()].clone()
        if n > special.numel():
            src[special.numel():] = torch.randn(n - special.numel(), generator=g)
        dst = _sent16(n + 8, T16)
        pkg.ops.cast_f32_bf16(src.cuda(), dst[:n])
        d = dst.cpu()
        want = src.to(T16)
        nan = torch.isnan(want)
        assert _same_bits(d[:n][~nan], want[~nan]), f"f32 -> {_name(T16)} n={n}: not torch's .to()"
        assert bool(torch.isnan(d[:n][nan]).all())
        nan_bits_same &= _same_bits(d[:n][nan], want[nan])
        assert bool((d[n:].view(I16) == SENT16).all()), f"cast n={n}: wrote past n"
    # 16-bit -> f32: every bit pattern (n = 65536), and short tails
    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(I16).view(T16)
    for n in [65536] + list(range(1, 18)) + [8 * 7 - 1, 8 * 7 + 1]:
        src = allb[torch.arange(n) * 997 % 65536].clone() if n < 65536 else allb
        out = torch.full((n + 4,), SENT32, dtype=F32, device="cuda")
        pkg.ops.cast_bf16_f32(src.cuda(), out[:n])
        o = out.cpu()
        want = src.to(F32)
        nan = torch.isnan(want)
        assert _same_bits(o[:n][~nan], want[~nan]) and bool(torch.isnan(o[:n][nan]).all()), f"{_name(T16)} -> f32 n={n}"
        nan_bits_same &= _same_bits(o[:n][nan], want[nan])
        assert bool((o[n:] == SENT32).all())
    _log(f"casts {_name(T16)}", {"f32<->16": "== torch .to() bit for bit", "nan_payloads_identical": nan_bits_same})


@DTYPES
@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_sum_shards(pkg, W, T16):
    g = torch.Generator().manual_seed(2200 + W)
    for shard in (8, 16, 8 * 257, 8 * 4099):
        x = (torch.randn(W, shard, generator=g) * 3).to(T16)
        if T16 == F16:
            x[:, :4] = 40000.0        # fp16: the f32 sum overflows the 16-bit maximum -> inf (W >= 2)
        out = _sent16(shard + 8, T16)
        pkg.ops.sum_shards_16(x.cuda(), out[:shard], W)
        acc = torch.zeros(shard, dtype=F32)
        for w in range(W):             # f32 sum in w order, rounded once
            acc = acc + x[w].to(F32)
        o = out.cpu()
        assert _same_bits(o[:shard], acc.to(T16)), f"sum_shards W{W} shard{shard}"
        assert bool((o[shard:].view(I16) == SENT16).all())
        if T16 == F16 and W >= 2:
            assert bool(torch.isinf(o[:4].to(F32)).all())
    _log(f"sum_shards W{W} {_name(T16)}", {"out": "== f32 sum in w order rounded once, bit for bit"})
