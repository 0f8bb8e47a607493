"""Every GEMM epilogue, LayerNorm and embedding / token-assembly path against one plain reference: float64 torch on the CPU,
computed from the same 16-bit tensors the kernels read.

The reference rounds to 16 bits exactly where a kernel stores 16 bits; f32 outputs, statistics and sums stay float64.  Dropout
masks are read back with ops.dropout_mask (the kernels' own hash) and injected into the reference.

Which path each case reaches (csrc/gemm.hip, csrc/layernorm.hip, csrc/embed.hip):

  case                                    kernel / host path
  ----------------------------------------------------------------------------------------------------------------------
  gemm_rounding (0,0) / (0,1) / (1,1)     mh_gemm_bf16_grouped: gemm_kernel<0,0,false> / <0,1,false> / <1,1,false>, integer
                                            operands whose f32 sums are exact but need more bits than the 16-bit significand:
                                            C, aux, + residual, alpha * acc + bias, each == exact.to(T16) bit for bit (RNE)
  gemm_fwd <shape>                        gemm_kernel<0,0,false> at the model's shapes (M 1 .. 6304, N 8 .. 3072, K 64 .. 4096)
  gemm_dgrad <shape>                      gemm_kernel<0,1,false>, contraction 768 / 3072, stored-derivative mul / residual
  gemm_wgrad T<n>                         gemm_kernel<1,1,false>, contraction T = 1 / 63 / 65 / 197 / 4103, f32 C, rowsum,
                                            alpha = 2^-13, MH_GEMM_ACCUM onto a nonzero C
  gemm_epilogue <combo>                   epilogue_rows: bias, aux, GELU / quick-GELU with and without MH_GEMM_DERIV_AUX, the dgrad
                                            multiply by a stored derivative or by gelu' / qgelu' of a stored pre-activation,
                                            residual, alpha; pre-activations spread over [-8, 8]
  gemm_dropout plain / packed             gemm_kernel<0,0,true>: drop, then drop_rows under rows_dev (mask index drop_rows[m] N + n)
  gemm_rows_dev (0,0) / (1,1)             rows_dev in {0, 1, 127, 129, M}: live-tile count (0,0), contraction clamp (1,1)
  gemm_grouped (0,0) / (0,1) / (1,1)      MH_GEMM_MAX_GROUP problems, packed and unpacked, several N == the single launches
  gemm_splitk K<n>                        ops.wgrad_splitk (split-K slabs + mh_colsum_partials_f32) at several
                                            mh_gemm_ksplit_for counts, K not a multiple of 64; == the unsplit launch within TOL_SUM
  gemm_partial_tiles (0,0) / (0,1)        N % 128 != 0, ldc > N, M % 128 != 0, every operand present; the [N, ldc) gap untouched
  ln_forward D<d>                         mh_layernorm_fwd_grouped: ln_fwd_kernel<NCH, 2>, NCH 1 / 2 / 4 / 8 (partial last chunk at
                                            D = 520 / 1032 / 2056), rows 1 / 7 / 8 / 9 / 197 / 4099, eps 1e-12 / 1e-6 / 1e-5,
                                            |mean|/std 0 .. 1000, constant and outlier rows
  ln_backward D<d>                        mh_layernorm_bwd_grouped: ln_bwd_kernel<NCH, DROP, 4>, NCH 1 / 2 / 4, dx_add, dx_drop with
                                            and without drop_rows, rows_dev (150 of 197 rows), n_part 1 / 3 / 8 / 16 (> rows) / 64,
                                            then mh_colsum_partials_f32 with scale != 1
  ln_grouped_fwd / _bwd D<d>              2 - 4 jobs with different rows, eps, rows_dev (0, partial, full) == the single-job
                                            launches bit for bit; one backward group mixes a dx_drop job with a plain one
  ln_env_variants rpw4 / bwd_waves8       ln_fwd_kernel<NCH, 4> (MEMEHIP_LN_FWD_RPW=4) and ln_bwd_kernel<NCH, ., 8>
                                            (MEMEHIP_LN_BWD_WAVES=8), read once per process: a subset of the cases above in a
                                            fresh child process per variant
  bert_embed_fwd D<d>                     bert_embed_fwd_kernel<NCH 1 / 2 / 4 / 8>: pre, in-register LayerNorm, dropout on y
  bert_embed_bwd <size> owner / indexed   bert_embed_bwd_word_kernel / bert_embed_index_kernel + _indexed_kernel,
                                            sum_over_batch_kernel, colsum_rows_f32_kernel; vocabulary 30522 x 32 x 128 tokens
  vit_assemble Np<n>                      vit_assemble_fwd_kernel; vit_assemble_bwd_copy_kernel + sum_over_batch_kernel + colsum

Bars, in units of the storage type's epsilon EPS (2^-10 fp16, 2^-7 bf16), with TOL_SUM = 1e-5:
  * stored 16-bit outputs: |hip - ref| <= 1 ulp(ref) + TOL_SUM x sum|terms|, where sum|terms| is the float64 sum of absolute
    products behind the value ((|A| |B|^T)[m, n] scaled by alpha, plus |bias|, |residual|, ...);
  * GELU-family outputs: sum|terms| of the pre-activation x is scaled by the largest |act'| (1.13) for the activation and by the
    largest |act''| (0.86) for a stored derivative, and the Abramowitz-Stegun erf bound of csrc/common.h gelu_parts is added:
    2e-7 |x| for the activation, 3e-7 for a derivative (stored, or recomputed from a stored pre-activation and multiplied in).
    The worst error where x < -3 (where 0.5 + 0.5 copysign(erf, x) cancels) is logged on its own line;
  * f32 outputs (f32 C, rowsum, ACCUM, summed split-K slabs, y_f32, dgamma / dbeta, embedding-table gradients): |hip - ref|
    <= TOL_SUM x sum|terms|;
  * statistics: mean within TOL_SUM x sum|x| / D; rstd within a relative EPS / 2 at EVERY |mean| / std tested (up to 1000: the
    forward variance is two-pass), nothing exempted;
  * bit-exact: the rounding-mode cases; y == y_f32.to(T16); constant rows give y == beta; grouped launches == separate launches;
    memory the kernel must not write (rows past M or the live count, columns [N, ldc)) keeps its sentinel.
y (LayerNorm, embedding) is checked against the apply step computed from the kernel's own mean / rstd, which are themselves checked
against float64: that isolates the apply arithmetic from the statistics.  The LayerNorm backward reads float64 statistics
rounded to f32; the reference uses those same f32 values.
Measured worst errors go through conftest.parity_log (profiles/r06_layer_paths_parity.txt).
"""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import parity_log

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64, I16, I32, I64 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int16, torch.int32, torch.int64
DTYPES = pytest.mark.parametrize("T16", [F16, BF16], ids=["fp16", "bf16"])
MANT = {F16: 10, BF16: 7}
EMIN = {F16: -14, BF16: -126}
TOL_SUM = 1e-5
LIP_ACT, LIP_DER = 1.13, 0.86        # max |act'|, max |act''| over both GELU forms
AS_ACT, AS_DER = 2e-7, 3e-7          # Abramowitz-Stegun erf bound carried through gelu_parts: per |x| / absolute
SENT16 = 0x7BAD                      # 16-bit sentinel bit pattern (finite in both types)
SENT32 = -7777.0
GSCALE = 8192.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = " ".join(f"{k.split('_', 2)[-1].lower()}={os.environ[k]}" for k in ("MEMEHIP_LN_FWD_RPW", "MEMEHIP_LN_BWD_WAVES")
                   if os.environ.get(k))


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_num_threads(16)
    import multimodal_propaganda_meme_classification_amd as m
    from multimodal_propaganda_meme_classification_amd import ops as _ops
    m.ops = _ops
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


def _uni(shape, g, lo, hi):
    return torch.rand(shape, generator=g, dtype=F64) * (hi - lo) + lo


def _sent16(shape, T16):
    return torch.full(shape, SENT16, dtype=I16, device="cuda").view(T16)


def _is_sent16(t):
    return bool((t.view(I16) == SENT16).all())


def _bits(t):
    return t.view(I16) if t.element_size() == 2 else t.view(I32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _rows_dev(n):
    return torch.tensor([n], dtype=I32, device="cuda")


def _rng(seed=4321, step=3):
    return torch.tensor([seed & 0x7FFFFFFF, (seed >> 31) & 0x7FFFFFFF, step, 0], dtype=I32, device="cuda")


def _drop_scale(p):
    """1 / (1 - p) as the kernels compute it in f32"""
    return float(torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32)))


def _mask(pkg, n, drop):
    return pkg.ops.dropout_mask(n, drop, "cuda").cpu().to(F64)


def _check16(what, got, ref, T16, slack=None, keep=None):
    """16-bit outputs: |got - ref| <= ulp(ref) + slack.  Returns the worst error as a fraction of the bar."""
    got = _cpu(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
    tol = _ulp(ref, T16) + (0.0 if slack is None else slack)
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


def _check_sum(what, got, ref, terms, tol=TOL_SUM, extra=None):
    """f32 outputs / sums: |got - ref| <= tol * sum|terms| (+ extra).  Returns the worst error as a fraction of the bar."""
    got = _cpu(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
    err = (got - ref).abs()
    bar = tol * terms + (0.0 if extra is None else extra) + 1e-30
    frac = err / bar
    worst = float(frac.max()) if frac.numel() else 0.0
    if worst > 1.0:
        i = int(frac.argmax())
        raise AssertionError(f"{what}: {int((frac > 1).sum())}/{frac.numel()} off; worst {worst:.3g} x bar "
                             f"(ref {float(ref.flatten()[i]):.6g}, got {float(got.flatten()[i]):.6g}, bar {float(bar.flatten()[i]):.3g})")
    return worst


def _log(tag, errs):
    v = f" [{VARIANT}]" if VARIANT else ""
    parity_log(f"[layer {tag}{v}] " + " ".join(f"{k} {x:.3e}" for k, x in errs.items()))


# ---------------------------------------------------------------------------------------------------------------------
# 1. GEMM
# ---------------------------------------------------------------------------------------------------------------------

LAYOUTS = pytest.mark.parametrize("layout", [(0, 0), (0, 1), (1, 1)], ids=["fwd00", "dgrad01", "wgrad11"])
SQ2 = math.sqrt(2.0)


def _phi(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _act(x, quick):
    if quick:
        return x * torch.sigmoid(1.702 * x)
    return x * 0.5 * (1.0 + torch.erf(x / SQ2))


def _dact(x, quick):
    if quick:
        s = torch.sigmoid(1.702 * x)
        return s * (1.0 + 1.702 * x * (1.0 - s))
    return 0.5 * (1.0 + torch.erf(x / SQ2)) + x * _phi(x)


def _operands(layout, M, N, K, g, T16, a_scale=1.0, b_scale=None):
    """A logical [M][K], B logical [N][K] (float64 holding 16-bit values) and their device forms with lda / ldb"""
    A = _r16(_rand((M, K), g, a_scale), T16)
    B = _r16(_rand((N, K), g, b_scale if b_scale is not None else 1.0 / math.sqrt(K)), T16)
    la, lb = layout      # a_kmajor: A stored [K][M]; b_kmajor: B stored [K][N]
    Ad = _dev((A.t() if la else A).contiguous(), T16)
    Bd = _dev((B.t() if lb else B).contiguous(), T16)
    lda = M if la else K
    ldb = N if lb else K
    return A, B, Ad, Bd, lda, ldb


def _mm(A, B):
    """float64 A B^T and |A| |B|^T"""
    return A @ B.t(), A.abs() @ B.abs().t()


def _epi_ref(acc, sabs, alpha=1.0, bias=None, dmask=None, act=None, quick=False, deriv_aux=False, mul=None, mul_kind=None,
             res=None):
    """float64 epilogue (include/memehip.h order).  Returns (aux_ref, aux_slack, out_ref, out_slack, pre) with slack the bar
    beyond 1 ulp; aux_ref None when no aux is stored under these flags."""
    v = alpha * acc
    tv = alpha * sabs
    if bias is not None:
        v = v + bias
        tv = tv + bias.abs()
    if dmask is not None:
        v = v * dmask
        tv = tv * dmask
    pre = v
    aux_ref = v
    aux_slack = TOL_SUM * tv
    extra = torch.zeros_like(v)
    if act is not None:
        if deriv_aux:
            aux_ref = _dact(v, quick)
            aux_slack = LIP_DER * TOL_SUM * tv + AS_DER
        extra = AS_ACT * v.abs()
        v = _act(v, quick)
        tv = LIP_ACT * tv
    if mul is not None:
        f = mul if mul_kind == "deriv" else _dact(mul, mul_kind == "qgelu")
        extra = extra * f.abs() + (0.0 if mul_kind == "deriv" else AS_DER * v.abs())
        v = v * f
        tv = tv * f.abs()
    if res is not None:
        v = v + res
        tv = tv + res.abs()
    return aux_ref, aux_slack, v, TOL_SUM * tv + extra, pre


def _tail(what, got, ref, slack, pre, T16):
    """the GELU tail x < -3: worst |hip - ref| (absolute) and as a fraction of the bar"""
    sel = pre < -3.0
    if not bool(sel.any()):
        return {}
    err = (_cpu(got) - ref).abs()[sel]
    bar = (_ulp(ref, T16) + slack)[sel]
    return {f"{what}_abs": float(err.max()), f"{what}_frac": float((err / bar).max()), f"{what}_n": float(sel.sum())}


# ---- 1a. rounding mode: exact integer sums that need more bits than the significand -------------------------------------

def _int_operands(M, N, K, T16, g):
    """A [M][K] in +-[1, 7] (a random sign per row), B [N][K] in [0, 7]; row 0 of A picks B[:, 0] + B[:, 1] = base + 0..7 (ties
    at base + 1, base + 3, ...) with base = 256 (bf16: first integer past the 8-bit significand) / 2048 (fp16)"""
    base = 256.0 if T16 == BF16 else 2048.0
    A = torch.randint(1, 8, (M, K), generator=g).to(F64)
    A *= torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0).to(F64)
    B = torch.randint(0, 8, (N, K), generator=g).to(F64)
    A[0] = 0.0
    A[0, :2] = 1.0
    B[:, 0] = base
    B[:, 1] = torch.arange(N, dtype=F64) % 8
    return A, B


@DTYPES
@LAYOUTS
def test_gemm_rounding_mode_exact(pkg, layout, T16):
    g = torch.Generator().manual_seed(11)
    M, N, K = 136, 256, (128 if T16 == BF16 else 256)
    A, B = _int_operands(M, N, K, T16, g)
    la, lb = layout
    Ad = _dev((A.t() if la else A).contiguous(), T16)
    Bd = _dev((B.t() if lb else B).contiguous(), T16)
    lda, ldb = (M if la else K), (N if lb else K)
    exact = A @ B.t()
    assert float(exact.abs().max()) < 2 ** 24       # every f32 partial sum is exact
    res = torch.randint(-64, 65, (M, N), generator=g).to(F64)
    bias = torch.randint(-100, 101, (N,), generator=g).to(F64)
    alpha = 0.25
    want = {"C": exact, "aux": exact, "C+res": exact + res, "alpha*C+bias": alpha * exact + bias}
    # the case must be able to tell RNE from truncation and from round-half-away
    for k, x in want.items():
        u = _ulp(x, T16)
        trunc = torch.sign(x) * torch.floor(x.abs() / u) * u
        away = torch.sign(x) * torch.floor(x.abs() / u + 0.5) * u
        assert bool((trunc != _r16(x, T16)).any()) and bool((away != _r16(x, T16)).any()), k
    C1, aux, C2 = (torch.empty((M, N), dtype=T16, device="cuda") for _ in range(3))
    C3 = torch.empty((M, N), dtype=T16, device="cuda")
    rd = _dev(res, T16)
    pkg.ops.gemm_grouped([pkg.ops.Gemm(Ad, Bd, C1, M, N, K, lda, ldb, N, aux=aux),
                          pkg.ops.Gemm(Ad, Bd, C2, M, N, K, lda, ldb, N, residual=rd),
                          pkg.ops.Gemm(Ad, Bd, C3, M, N, K, lda, ldb, N, bias=bias.to(F32).cuda(), alpha=alpha)], la, lb)
    torch.cuda.synchronize()
    ties = 0
    for k, got in (("C", C1), ("aux", aux), ("C+res", C2), ("alpha*C+bias", C3)):
        x = want[k]
        w = x.to(T16)
        u = _ulp(x, T16)
        ties += int(((x.abs() / u) % 1 == 0.5).sum())
        if not _same_bits(got.cpu(), w):
            bad = got.cpu().to(F64) != w.to(F64)
            i = int(bad.flatten().nonzero()[0])
            raise AssertionError(f"{k}: {int(bad.sum())}/{bad.numel()} stores are not round-to-nearest-even "
                                 f"(exact {float(x.flatten()[i])}, got {float(got.cpu().flatten()[i].float())}, want {float(w.flatten()[i].float())})")
    assert ties > 100
    parity_log(f"[layer gemm_rounding {layout[0]}{layout[1]} {_name(T16)}] C, aux, C+res, alpha*C+bias == RNE bit for bit ({ties} ties)")


# ---- 1b. real-valued layouts at the model's shapes ------------------------------------------------------------------------

FWD_SHAPES = {      # name: (M, N, K, bias, residual)
    "vit_ffn_up_6304x3072x768": (6304, 3072, 768, True, False),
    "text_ffn_down_4096x768x3072": (4096, 768, 3072, True, True),
    "qkv_394x2304x768": (394, 2304, 768, True, False),
    "M1_N8_K64": (1, 8, 64, True, True),
    "M127_N120_K4096": (127, 120, 4096, False, True),
    "M129_N768_K64": (129, 768, 64, True, False),
}


@DTYPES
@pytest.mark.parametrize("case", list(FWD_SHAPES))
def test_gemm_fwd_shapes(pkg, case, T16):
    M, N, K, has_b, has_r = FWD_SHAPES[case]
    g = torch.Generator().manual_seed(list(FWD_SHAPES).index(case))
    A, B, Ad, Bd, lda, ldb = _operands((0, 0), M, N, K, g, T16)
    bias = _rand((N,), g, 0.5).to(F32).to(F64) if has_b else None
    res = _r16(_rand((M, N), g), T16) if has_r else None
    C = torch.empty((M, N), dtype=T16, device="cuda")
    pkg.ops.gemm_grouped([pkg.ops.Gemm(Ad, Bd, C, M, N, K, lda, ldb, N, bias=None if bias is None else bias.to(F32).cuda(),
                                       residual=None if res is None else _dev(res, T16))], False, False)
    acc, sabs = _mm(A, B)
    _, _, ref, slack, _ = _epi_ref(acc, sabs, bias=bias, res=res)
    e = _check16(f"fwd {case} C", C, ref, T16, slack)
    _log(f"gemm_fwd {case} {_name(T16)}", {"C": e})


DGRAD_SHAPES = {    # name: (M, N, K, mul, residual): out[M][N] = dy[M][K] W[K][N]
    "ffn_down_dgrad_4096x3072x768_mul": (4096, 3072, 768, True, False),
    "ffn_up_dgrad_6304x768x3072_res": (6304, 768, 3072, False, True),
    "M129_N264_K768_mul_res": (129, 264, 768, True, True),
}


@DTYPES
@pytest.mark.parametrize("case", list(DGRAD_SHAPES))
def test_gemm_dgrad_shapes(pkg, case, T16):
    M, N, K, has_m, has_r = DGRAD_SHAPES[case]
    g = torch.Generator().manual_seed(20 + list(DGRAD_SHAPES).index(case))
    A, B, Ad, Bd, lda, ldb = _operands((0, 1), M, N, K, g, T16)
    mul = _r16(_dact(_uni((M, N), g, -8, 8), False), T16) if has_m else None
    res = _r16(_rand((M, N), g), T16) if has_r else None
    C = torch.empty((M, N), dtype=T16, device="cuda")
    pkg.ops.gemm_grouped([pkg.ops.Gemm(Ad, Bd, C, M, N, K, lda, ldb, N, mul=None if mul is None else _dev(mul, T16),
                                       residual=None if res is None else _dev(res, T16), deriv_aux=has_m)], False, True)
    acc, sabs = _mm(A, B)
    _, _, ref, slack, _ = _epi_ref(acc, sabs, mul=mul, mul_kind="deriv", res=res)
    e = _check16(f"dgrad {case} C", C, ref, T16, slack)
    _log(f"gemm_dgrad {case} {_name(T16)}", {"C": e})


WGRAD_SHAPES = {    # name: (M = N_out, N = K_in, T, accum)
    "T1": (128, 256, 1, False),
    "T63": (256, 128, 63, True),
    "T65": (768, 768, 65, False),
    "T197": (3072, 768, 197, True),
    "T4103": (768, 768, 4103, True),
}


@DTYPES
@pytest.mark.parametrize("case", list(WGRAD_SHAPES))
def test_gemm_wgrad_shapes(pkg, case, T16):
    M, N, T, accum = WGRAD_SHAPES[case]
    g = torch.Generator().manual_seed(7 + T)
    alpha = 1.0 / GSCALE
    dy = _r16(_rand((M, T), g, 64.0), T16)          # logical [N_out][T]: the loss-scaled gradient stream
    x = _r16(_rand((N, T), g), T16)
    Ad = _dev(dy.t().contiguous(), T16)             # stored [T][N_out]
    Bd = _dev(x.t().contiguous(), T16)              # stored [T][K_in]
    C0 = _rand((M, N), g, 0.3).to(F32).to(F64) if accum else None
    C = (C0.to(F32).cuda() if accum else torch.full((M, N), SENT32, dtype=F32, device="cuda"))
    rowsum = torch.full((M,), SENT32, dtype=F32, device="cuda")
    pkg.ops.gemm_grouped([pkg.ops.Gemm(Ad, Bd, C, M, N, T, M, N, N, rowsum=rowsum, accum=accum, alpha=alpha)], True, True)
    acc, sabs = _mm(dy, x)
    ref = alpha * acc + (C0 if accum else 0.0)
    terms = alpha * sabs + (C0.abs() if accum else 0.0)
    e_c = _check_sum(f"wgrad {case} C", C, ref, terms)
    e_r = _check_sum(f"wgrad {case} rowsum", rowsum, alpha * dy.sum(1), alpha * dy.abs().sum(1))
    _log(f"gemm_wgrad {case} {_name(T16)}", {"C": e_c, "rowsum": e_r})


# ---- 1c. every epilogue combination the engine issues -----------------------------------------------------------------

EPI_M, EPI_N, EPI_K = 264, 768, 768
FWD_EPI = {         # name: (gelu, quick, deriv_aux, aux, residual, alpha)
    "bias": (False, False, False, False, False, 1.0),
    "bias_aux": (False, False, False, True, False, 1.0),
    "gelu": (True, False, False, False, False, 1.0),
    "gelu_aux": (True, False, False, True, False, 1.0),
    "gelu_deriv_aux": (True, False, True, True, False, 1.0),
    "qgelu": (True, True, False, False, False, 1.0),
    "qgelu_aux": (True, True, False, True, False, 1.0),
    "qgelu_deriv_aux": (True, True, True, True, False, 1.0),
    "bias_res": (False, False, False, False, True, 1.0),
    "alpha_bias_res": (False, False, False, False, True, 0.125),
}
DGRAD_EPI = {       # name: (mul kind, residual)
    "mul_deriv": ("deriv", False),
    "mul_gelu": ("gelu", False),
    "mul_qgelu": ("qgelu", False),
    "mul_deriv_res": ("deriv", True),
    "mul_gelu_res": ("gelu", True),
    "mul_qgelu_res": ("qgelu", True),
    "res": (None, True),
}
_EPI_CACHE = {}


def _epi_operands(T16, layout):
    key = (T16, layout)
    if key not in _EPI_CACHE:
        g = torch.Generator().manual_seed(99 + layout[1])
        A, B, Ad, Bd, lda, ldb = _operands(layout, EPI_M, EPI_N, EPI_K, g, T16)
        acc, sabs = _mm(A, B)
        extra = dict(bias=_uni((EPI_N,), g, -8, 8).to(F32).to(F64),           # pre-activations over [-8, 8]: the tails
                     res=_r16(_rand((EPI_M, EPI_N), g), T16),
                     pre=_r16(_uni((EPI_M, EPI_N), g, -8, 8), T16))
        _EPI_CACHE[key] = (Ad, Bd, lda, ldb, acc, sabs, extra)
    return _EPI_CACHE[key]


@DTYPES
@pytest.mark.parametrize("combo", list(FWD_EPI))
def test_gemm_epilogue_forward(pkg, combo, T16):
    gelu, quick, deriv, has_aux, has_res, alpha = FWD_EPI[combo]
    Ad, Bd, lda, ldb, acc, sabs, ex = _epi_operands(T16, (0, 0))
    M, N, K = EPI_M, EPI_N, EPI_K
    C = torch.empty((M, N), dtype=T16, device="cuda")
    aux = torch.empty((M, N), dtype=T16, device="cuda") if has_aux else None
    res = ex["res"] if has_res else None
    pkg.ops.gemm_grouped([pkg.ops.Gemm(Ad, Bd, C, M, N, K, lda, ldb, N, bias=ex["bias"].to(F32).cuda(), aux=aux,
                                       residual=None if res is None else _dev(res, T16), gelu=gelu, quick=quick, deriv_aux=deriv,
                                       alpha=alpha)], False, False)
    aux_ref, aux_slack, ref, slack, pre = _epi_ref(acc, sabs, alpha=alpha, bias=ex["bias"], act=("q" if quick else "e") if gelu else None,
                                                   quick=quick, deriv_aux=deriv, res=res)
    errs = {"C": _check16(f"{combo} C", C, ref, T16, slack)}
    if has_aux:
        errs["aux"] = _check16(f"{combo} aux", aux, aux_ref, T16, aux_slack)
    _log(f"gemm_epilogue fwd {combo} {_name(T16)}", errs)
    if gelu:
        tails = _tail("C", C, ref, slack, pre, T16)
        if deriv:
            tails.update(_tail("aux", aux, aux_ref, aux_slack, pre, T16))
        _log(f"gemm_epilogue fwd {combo} {_name(T16)} tail x<-3", tails)


@DTYPES
@pytest.mark.parametrize("combo", list(DGRAD_EPI))
def test_gemm_epilogue_dgrad(pkg, combo, T16):
    kind, has_res = DGRAD_EPI[combo]
    Ad, Bd, lda, ldb, acc, sabs, ex = _epi_operands(T16, (0, 1))
    M, N, K = EPI_M, EPI_N, EPI_K
    if kind == "deriv":
        mul = _r16(_dact(ex["pre"], False), T16)      # the stored derivative of a DERIV_AUX forward
    elif kind is not None:
        mul = ex["pre"]                               # the stored pre-activation
    else:
        mul = None
    res = ex["res"] if has_res else None
    C = torch.empty((M, N), dtype=T16, device="cuda")
    pkg.ops.gemm_grouped([pkg.ops.Gemm(Ad, Bd, C, M, N, K, lda, ldb, N, mul=None if mul is None else _dev(mul, T16),
                                       residual=None if res is None else _dev(res, T16), quick=kind == "qgelu",
                                       deriv_aux=kind == "deriv")], False, True)
    _, _, ref, slack, _ = _epi_ref(acc, sabs, mul=mul, mul_kind=kind, res=res)
    errs = {"C": _check16(f"{combo} C", C, ref, T16, slack)}
    _log(f"gemm_epilogue dgrad {combo} {_name(T16)}", errs)
    if kind in ("gelu", "qgelu"):
        _log(f"gemm_epilogue dgrad {combo} {_name(T16)} tail x<-3", _tail("C", C, ref, slack, ex["pre"], T16))


# ---- 1d. dropout epilogue ---------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("mode", ["plain", "packed"])
def test_gemm_dropout(pkg, mode, T16):
    M, N, K, U, live = 300, 768, 768, 512, 257
    g = torch.Generator().manual_seed(5)
    A, B, Ad, Bd, lda, ldb = _operands((0, 0), M, N, K, g, T16)
    bias = _rand((N,), g, 0.5).to(F32).to(F64)
    res = _r16(_rand((M, N), g), T16)
    drop = (_rng(), 0.1, 17)
    C = _sent16((M, N), T16)
    if mode == "packed":
        rows = torch.sort(torch.randperm(U, generator=g)[:M]).values
        rows_dev, drop_rows = _rows_dev(live), rows.to(I32).cuda()
        n_live = live
    else:
        rows, rows_dev, drop_rows, n_live = torch.arange(M), None, None, M
    pkg.ops.gemm_grouped([pkg.ops.Gemm(Ad, Bd, C, M, N, K, lda, ldb, N, bias=bias.to(F32).cuda(), residual=_dev(res, T16),
                                       drop=drop, rows_dev=rows_dev, drop_rows=drop_rows)], False, False)
    mask = _mask(pkg, U * N, drop).view(U, N)[rows] * _drop_scale(drop[1])
    assert 0.85 < float((mask > 0).to(F64).mean()) < 0.95
    acc, sabs = _mm(A, B)
    _, _, ref, slack, _ = _epi_ref(acc, sabs, bias=bias, dmask=mask, res=res)
    e = _check16(f"dropout {mode} C", C[:n_live], ref[:n_live], T16, slack[:n_live])
    assert _is_sent16(C[n_live:]), "rows past the live count were written"
    _log(f"gemm_dropout {mode} {_name(T16)}", {"C": e})


# ---- 1e. packed rows ----------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("live", [0, 1, 127, 129, 394])
def test_gemm_rows_dev_forward(pkg, live, T16):
    M, N, K = 394, 256, 128
    g = torch.Generator().manual_seed(31)
    A, B, Ad, Bd, lda, ldb = _operands((0, 0), M, N, K, g, T16)
    bias = _rand((N,), g, 0.5).to(F32).to(F64)
    C, aux = _sent16((M, N), T16), _sent16((M, N), T16)
    pkg.ops.gemm_grouped([pkg.ops.Gemm(Ad, Bd, C, M, N, K, lda, ldb, N, bias=bias.to(F32).cuda(), aux=aux, gelu=True,
                                       rows_dev=_rows_dev(live))], False, False)
    acc, sabs = _mm(A[:live], B)
    aux_ref, aux_slack, ref, slack, _ = _epi_ref(acc, sabs, bias=bias, act="e")
    errs = {}
    if live:
        errs["C"] = _check16("rows_dev C", C[:live], ref, T16, slack)
        errs["aux"] = _check16("rows_dev aux", aux[:live], aux_ref, T16, aux_slack)
    assert _is_sent16(C[live:]) and _is_sent16(aux[live:]), "rows past the live count were written"
    _log(f"gemm_rows_dev fwd00 live={live} {_name(T16)}", errs or {"sentinel_only": 0.0})


@DTYPES
@pytest.mark.parametrize("live", [0, 1, 127, 129, 394])
def test_gemm_rows_dev_wgrad(pkg, live, T16):
    M, N, T = 256, 128, 394       # dW[M][N] = dy^T x over the first `live` of T packed rows
    g = torch.Generator().manual_seed(37)
    dy = _r16(_rand((T, M), g, 64.0), T16)
    x = _r16(_rand((T, N), g), T16)
    dy[live:] = 4096.0                 # rows past the live count: must not enter the sums
    x[live:] = -3000.0
    alpha = 1.0 / GSCALE
    C = torch.full((M, N), SENT32, dtype=F32, device="cuda")
    rowsum = torch.full((M,), SENT32, dtype=F32, device="cuda")
    pkg.ops.gemm_grouped([pkg.ops.Gemm(_dev(dy, T16), _dev(x, T16), C, M, N, T, M, N, N, rowsum=rowsum, alpha=alpha,
                                       rows_dev=_rows_dev(live))], True, True)
    d, xx = dy[:live], x[:live]
    e_c = _check_sum("rows_dev wgrad C", C, alpha * d.t() @ xx, alpha * d.abs().t() @ xx.abs())
    e_r = _check_sum("rows_dev wgrad rowsum", rowsum, alpha * d.sum(0), alpha * d.abs().sum(0))
    _log(f"gemm_rows_dev wgrad11 live={live} {_name(T16)}", {"C": e_c, "rowsum": e_r})


def _group_problems(pkg, layout, T16, g):
    """MH_GEMM_MAX_GROUP problems of one layout: several N, packed (rows_dev) and unpacked, different epilogues"""
    la, lb = layout
    specs = [(394, 768, 128, None), (200, 2304, 64, 150), (129, 120, 192, None), (64, 256, 128, 0),
             (300, 8, 64, 300), (1, 136, 64, None), (257, 384, 128, 129), (128, 768, 64, None)]
    probs, outs = [], []
    for i, (M, N, K, live) in enumerate(specs):
        if la:
            M = (M + 7) // 8 * 8
        A, B, Ad, Bd, lda, ldb = _operands(layout, M, N, K, g, T16)
        kw = {}
        if la == 1:
            C = torch.full((M, N), SENT32, dtype=F32, device="cuda")
            kw["rowsum"] = torch.full((M,), SENT32, dtype=F32, device="cuda")
            kw["alpha"] = 1.0 / GSCALE
            kw["accum"] = i % 2 == 1
        else:
            C = _sent16((M, N), T16)
            if i % 2 == 0:
                kw["residual"] = _dev(_rand((M, N), g), T16)
            if lb == 0:
                kw["bias"] = _rand((N,), g).to(F32).cuda()
                if i % 3 == 0:
                    kw.update(aux=_sent16((M, N), T16), gelu=True, deriv_aux=i % 2 == 0, quick=i == 3)
            else:
                kw["mul"] = _dev(_uni((M, N), g, -4, 4), T16)
                kw["quick"] = i == 5
        if live is not None:
            kw["rows_dev"] = _rows_dev(live)
        probs.append(dict(Ad=Ad, Bd=Bd, C=C, M=M, N=N, K=K, lda=lda, ldb=ldb, kw=kw))
    return probs


def _clone_out(p):
    q = dict(p)
    q["C"] = p["C"].clone()
    q["kw"] = dict(p["kw"])
    for k in ("aux", "rowsum"):
        if k in q["kw"]:
            q["kw"][k] = p["kw"][k].clone()
    return q


def _gemm_of(pkg, p):
    return pkg.ops.Gemm(p["Ad"], p["Bd"], p["C"], p["M"], p["N"], p["K"], p["lda"], p["ldb"], p["N"], **p["kw"])


@DTYPES
@LAYOUTS
def test_gemm_grouped_equals_single(pkg, layout, T16):
    g = torch.Generator().manual_seed(41 + 3 * layout[0] + layout[1])
    probs = _group_problems(pkg, layout, T16, g)
    single = [_clone_out(p) for p in probs]
    assert len(probs) == pkg._lib.MH_GEMM_MAX_GROUP
    pkg.ops.gemm_grouped([_gemm_of(pkg, p) for p in probs], *layout)
    for q in single:
        pkg.ops.gemm_grouped([_gemm_of(pkg, q)], *layout)
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(probs, single)):
        assert _same_bits(p["C"], q["C"]), f"problem {i}: grouped C differs from the single launch"
        for k in ("aux", "rowsum"):
            if k in p["kw"]:
                assert _same_bits(p["kw"][k], q["kw"][k]), f"problem {i}: grouped {k} differs from the single launch"
        live = p["kw"].get("rows_dev")
        if live is not None and layout[0] == 0:
            n = int(live.item())
            assert _is_sent16(p["C"][n:]), f"problem {i}: rows past the live count were written"
    parity_log(f"[layer gemm_grouped {layout[0]}{layout[1]} {_name(T16)}] {len(probs)} problems == single launches bit for bit")


# ---- 1f. split-K ------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("K", [1000, 4103, 6304])
def test_gemm_splitk(pkg, K, T16):
    M, N = 256, 384
    g = torch.Generator().manual_seed(K)
    alpha = 1.0 / GSCALE
    dy = _r16(_rand((K, M), g, 64.0), T16)
    x = _r16(_rand((K, N), g), T16)
    dyd, xd = _dev(dy, T16), _dev(x, T16)
    ref, terms = alpha * dy.t() @ x, alpha * dy.abs().t() @ x.abs()
    whole = torch.empty((M, N), dtype=F32, device="cuda")
    pkg.ops.gemm_grouped([pkg.ops.Gemm(dyd, xd, whole, M, N, K, M, N, N, alpha=alpha)], True, True)
    errs = {"unsplit": _check_sum("unsplit", whole, ref, terms)}
    lib = _lib(pkg, T16)
    seen = set()
    for want in (2, 3, 5, 16, 64):
        sp = lib.mh_gemm_ksplit_for(K, min(want, max(1, K // 256)))
        if sp in seen or sp <= 1:
            continue
        seen.add(sp)
        out = pkg.ops.wgrad_splitk(dyd, xd, M, N, K, M, N, alpha=alpha, target_tiles=10 ** 6, max_split=sp)
        errs[f"split{sp}"] = _check_sum(f"split-K {sp}", out, ref, terms)
        errs[f"split{sp}_vs_unsplit"] = _check_sum(f"split-K {sp} vs unsplit", out, _cpu(whole), terms)
    assert len(seen) >= 2, seen
    _log(f"gemm_splitk K={K} {_name(T16)}", errs)


# ---- 1g. partial tiles ------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("layout", [(0, 0), (0, 1)], ids=["fwd00", "dgrad01"])
@pytest.mark.parametrize("N", [120, 264])
def test_gemm_partial_tiles(pkg, layout, N, T16):
    M, K = 200, 192
    ldc = N + 16
    g = torch.Generator().manual_seed(N + layout[1])
    A, B, Ad, Bd, lda, ldb = _operands(layout, M, N, K, g, T16)
    bias = _uni((N,), g, -8, 8).to(F32).to(F64)
    res = _r16(_rand((M, N), g), T16)
    resd = _sent16((M, ldc), T16)
    resd[:, :N] = _dev(res, T16)
    C, aux = _sent16((M, ldc), T16), _sent16((M, ldc), T16)
    acc, sabs = _mm(A, B)
    if layout == (0, 0):
        pkg.ops.gemm_grouped([pkg.ops.Gemm(Ad, Bd, C, M, N, K, lda, ldb, ldc, bias=bias.to(F32).cuda(), aux=aux, residual=resd,
                                           gelu=True, deriv_aux=True)], False, False)
        aux_ref, aux_slack, ref, slack, _ = _epi_ref(acc, sabs, bias=bias, act="e", deriv_aux=True, res=res)
        errs = {"C": _check16("partial C", C[:, :N], ref, T16, slack),
                "aux": _check16("partial aux", aux[:, :N], aux_ref, T16, aux_slack)}
        assert _is_sent16(aux[:, N:]), "aux columns [N, ldc) were written"
    else:
        pre = _r16(_uni((M, N), g, -6, 6), T16)
        muld = _sent16((M, ldc), T16)
        muld[:, :N] = _dev(pre, T16)
        pkg.ops.gemm_grouped([pkg.ops.Gemm(Ad, Bd, C, M, N, K, lda, ldb, ldc, mul=muld, residual=resd)], False, True)
        _, _, ref, slack, _ = _epi_ref(acc, sabs, mul=pre, mul_kind="gelu", res=res)
        errs = {"C": _check16("partial C", C[:, :N], ref, T16, slack)}
    assert _is_sent16(C[:, N:]), "C columns [N, ldc) were written"
    _log(f"gemm_partial_tiles {layout[0]}{layout[1]} N={N} ldc={ldc} M={M} {_name(T16)}", errs)


# ---------------------------------------------------------------------------------------------------------------------
# 2. LayerNorm
# ---------------------------------------------------------------------------------------------------------------------

LN_DS = (8, 64, 504, 512, 520, 768, 1024, 1032, 2048, 2056, 3072, 4096)
LN_EPS = (1e-12, 1e-6, 1e-5)
LN_ROWS = (1, 7, 8, 9, 197)
ROW_KINDS = ("randn", "r0", "r10", "r100", "r1000", "const", "outlier")


def _ln_input(rows, D, g, T16, kinds=ROW_KINDS):
    """16-bit rows cycling through `kinds`: randn; |mean| / std = 0 / 10 / 100 / 1000; constant; one outlier of 1000 std"""
    x = torch.empty((rows, D), dtype=F64)
    for i in range(rows):
        k = kinds[i % len(kinds)]
        std = float(torch.rand(1, generator=g)) * 1.5 + 0.5
        sgn = 1.0 if float(torch.rand(1, generator=g)) < 0.5 else -1.0
        z = torch.randn(D, generator=g, dtype=F64)
        if k == "randn":
            x[i] = z * std + 0.3 * sgn
        elif k[0] == "r":
            x[i] = (z - z.mean()) * std + sgn * float(k[1:]) * std
        elif k == "const":
            x[i] = sgn * (1.0 + float(torch.rand(1, generator=g)))
        else:
            x[i] = z * std
            x[i, int(torch.randint(0, D, (1,), generator=g))] = sgn * 1000.0 * std
    return _r16(x, T16), [kinds[i % len(kinds)] for i in range(rows)]


def _ln_stats(x, eps):
    mu = x.mean(1)
    var = ((x - mu[:, None]) ** 2).mean(1)
    return mu, 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=F32)))


def _ln_fwd_launch(pkg, T16, D, jobs):
    """jobs: dicts with x (device), gamma, beta (device f32), rows, eps, rows_dev; allocates sentinel-filled outputs"""
    arr = (pkg._lib.MhLnFwdJob * len(jobs))()
    for e, j in zip(arr, jobs):
        R = j["rows"]
        j.setdefault("y", _sent16((R, D), T16))
        j.setdefault("y32", torch.full((R, D), SENT32, dtype=F32, device="cuda"))
        j.setdefault("mean", torch.full((R,), SENT32, dtype=F32, device="cuda"))
        j.setdefault("rstd", torch.full((R,), SENT32, dtype=F32, device="cuda"))
        e.x, e.gamma, e.beta, e.y, e.y_f32 = j["x"].data_ptr(), j["gamma"].data_ptr(), j["beta"].data_ptr(), j["y"].data_ptr(), j["y32"].data_ptr()
        e.mean, e.rstd, e.rows, e.eps = j["mean"].data_ptr(), j["rstd"].data_ptr(), R, float(j["eps"])
        e.rows_dev = None if j.get("rows_dev") is None else j["rows_dev"].data_ptr()
    pkg._lib.check(_lib(pkg, T16).mh_layernorm_fwd_grouped(arr, len(jobs), D, _st()), "mh_layernorm_fwd_grouped")
    torch.cuda.synchronize()
    return jobs


def _check_ln_forward(tag, T16, x, kinds, gamma, beta, eps, j, n):
    """rows [0, n) against float64, rows [n, rows) still the sentinel"""
    eps16 = _eps(T16)
    x = x[:n]
    mu, rstd = _ln_stats(x, eps)
    m_k, r_k = _cpu(j["mean"][:n]), _cpu(j["rstd"][:n])
    errs = {"mean": _check_sum(f"{tag} mean", j["mean"][:n], mu, x.abs().mean(1)) if n else 0.0}
    rel = (r_k - rstd).abs() / rstd
    e_rstd = float(rel.max()) if n else 0.0
    assert e_rstd <= eps16 / 2, f"{tag} rstd: relative error {e_rstd:.3g} > EPS/2 = {eps16 / 2:.3g} (row kind {kinds[int(rel.argmax())]})"
    errs["rstd"] = e_rstd / (eps16 / 2)
    for kd in ("r100", "r1000"):
        sel = torch.tensor([k == kd for k in kinds[:n]], dtype=torch.bool)
        if sel.any():
            errs[f"rstd_{kd}"] = float(rel[sel].max()) / (eps16 / 2)
    d = x - m_k[:, None]
    v = d * r_k[:, None] * gamma + beta
    terms = (d * r_k[:, None] * gamma).abs() + beta.abs()
    errs["y_f32"] = _check_sum(f"{tag} y_f32", j["y32"][:n], v, terms)
    errs["y"] = _check16(f"{tag} y", j["y"][:n], v, T16, TOL_SUM * terms)
    y, y32 = j["y"][:n].cpu(), j["y32"][:n].cpu()
    assert _same_bits(y, y32.to(T16)), f"{tag}: y != y_f32.to(T16)"
    const = torch.tensor([k == "const" for k in kinds[:n]], dtype=torch.bool)
    if const.any():
        assert torch.equal(y32[const].to(F64), beta.expand(int(const.sum()), -1)), f"{tag}: a constant row's y_f32 != beta"
        assert _same_bits(y[const], beta.to(T16).expand(int(const.sum()), -1).contiguous()), f"{tag}: a constant row's y != beta"
    R = j["rows"]
    if n < R:
        assert _is_sent16(j["y"][n:]), f"{tag}: y rows past the live count were written"
        for k in ("y32", "mean", "rstd"):
            assert bool((j[k][n:] == SENT32).all()), f"{tag}: {k} rows past the live count were written"
    return errs


def _ln_params(D, g):
    gamma = (1.0 + 0.2 * _rand((D,), g)).to(F32).to(F64)
    beta = (0.3 * _rand((D,), g)).to(F32).to(F64)
    return gamma, beta


@DTYPES
@pytest.mark.parametrize("D", LN_DS, ids=[f"D{d}" for d in LN_DS])
def test_ln_forward(pkg, D, T16):
    g = torch.Generator().manual_seed(D)
    eps = LN_EPS[LN_DS.index(D) % 3]
    R = 4099
    x, kinds = _ln_input(R, D, g, T16)
    gamma, beta = _ln_params(D, g)
    xd, gd, bd = _dev(x, T16), gamma.to(F32).cuda(), beta.to(F32).cuda()
    big = _ln_fwd_launch(pkg, T16, D, [dict(x=xd, gamma=gd, beta=bd, rows=R, eps=eps)])[0]
    errs = _check_ln_forward(f"ln_fwd D={D}", T16, x, kinds, gamma, beta, eps, big, R)
    _log(f"ln_forward D={D} rows={R} eps={eps:g} {_name(T16)}", errs)
    for r in LN_ROWS:      # small launches: a row is computed the same way whatever the launch, so they equal the big one's rows
        j = _ln_fwd_launch(pkg, T16, D, [dict(x=xd[:r].contiguous(), gamma=gd, beta=bd, rows=r, eps=eps)])[0]
        for k in ("y", "y32", "mean", "rstd"):
            assert _same_bits(j[k], big[k][:r]), f"rows={r}: {k} differs from the same rows of the {R}-row launch"


def _ln_bwd_launch(pkg, T16, D, jobs):
    arr = (pkg._lib.MhLnBwdJob * len(jobs))()
    for e, j in zip(arr, jobs):
        R = j["rows"]
        j.setdefault("dx", _sent16((R, D), T16))
        j.setdefault("part", torch.full((2, j["n_part"], D), SENT32, dtype=F32, device="cuda"))
        if j.get("drop") is not None:
            j.setdefault("dx_drop", _sent16((R, D), T16))
        p = lambda t: None if t is None else t.data_ptr()
        e.dy, e.x, e.gamma, e.mean, e.rstd = p(j["dy"]), p(j["x"]), p(j["gamma"]), p(j["mean"]), p(j["rstd"])
        e.dx_add, e.dx, e.part, e.dx_drop = p(j.get("dx_add")), p(j["dx"]), p(j["part"]), p(j.get("dx_drop"))
        drop = j.get("drop")
        e.rng = None if drop is None else drop[0].data_ptr()
        e.drop_p, e.drop_stream = (0.0, 0) if drop is None else (float(drop[1]), int(drop[2]))
        e.n_part, e.rows = j["n_part"], R
        e.rows_dev, e.drop_rows = p(j.get("rows_dev")), p(j.get("drop_rows"))
    pkg._lib.check(_lib(pkg, T16).mh_layernorm_bwd_grouped(arr, len(jobs), D, _st()), "mh_layernorm_bwd_grouped")
    torch.cuda.synchronize()
    return jobs


def _ln_bwd_waves():
    """rows per workgroup step of ln_bwd_kernel: its wave count (MEMEHIP_LN_BWD_WAVES=8, else 4)"""
    return 8 if os.environ.get("MEMEHIP_LN_BWD_WAVES") == "8" else 4


def _ln_bwd_ref(x, dy, gamma, m, r, add=None):
    """float64 LayerNorm backward from the 16-bit x / dy and the statistics the kernel reads"""
    xh = (x - m[:, None]) * r[:, None]
    dyg = dy * gamma
    c1 = dyg.mean(1, keepdim=True)
    c2 = (dyg * xh).mean(1, keepdim=True)
    dx = r[:, None] * (dyg - c1 - xh * c2)
    terms = r[:, None] * (dyg.abs() + dyg.abs().mean(1, keepdim=True) + xh.abs() * (dyg * xh).abs().mean(1, keepdim=True))
    if add is not None:
        dx = dx + add
        terms = terms + add.abs()
    return dx, terms, xh


def _ln_bwd_case(pkg, T16, D, rows, n_part, g, eps, add=False, drop=False, drop_rows=False, live=None, scale=1.0, kinds=None):
    """one backward job + mh_colsum_partials_f32; returns (errs, job, host operands)"""
    if kinds is None:
        kinds = ("randn", "r0", "r10", "outlier") + (("const",) if (T16 == BF16 or eps >= 1e-6) else ())
    x, kinds_r = _ln_input(rows, D, g, T16, kinds)
    gamma, _ = _ln_params(D, g)
    mu, rs = _ln_stats(x, eps)
    m32, r32 = mu.to(F32), rs.to(F32)
    dy = _r16(_rand((rows, D), g), T16)
    dxa = _r16(_rand((rows, D), g), T16) if add else None
    n = rows if live is None else live
    U = 2 * rows + 5
    dmap = torch.sort(torch.randperm(U, generator=g)[:rows]).values if drop_rows else torch.arange(rows)
    dr = (_rng(77, 9), 0.1, 23) if drop else None
    j = dict(dy=_dev(dy, T16), x=_dev(x, T16), gamma=gamma.to(F32).cuda(), mean=m32.cuda(), rstd=r32.cuda(),
             dx_add=None if dxa is None else _dev(dxa, T16), n_part=n_part, rows=rows, drop=dr,
             rows_dev=None if live is None else _rows_dev(live), drop_rows=dmap.to(I32).cuda() if drop_rows else None)
    _ln_bwd_launch(pkg, T16, D, [j])
    tag = f"ln_bwd D={D} rows={rows} n_part={n_part}"
    m64, r64 = m32.to(F64)[:n], r32.to(F64)[:n]
    dx, terms, xh = _ln_bwd_ref(x[:n], dy[:n], gamma, m64, r64, None if dxa is None else dxa[:n])
    errs = {"dx": _check16(f"{tag} dx", j["dx"][:n], dx, T16, TOL_SUM * terms)}
    if drop:
        mk = _mask(pkg, U * D, dr).view(U, D)[dmap[:n]] * _drop_scale(dr[1])
        errs["dx_drop"] = _check16(f"{tag} dx_drop", j["dx_drop"][:n], dx * mk, T16, TOL_SUM * terms * mk)
        assert _is_sent16(j["dx_drop"][n:]), f"{tag}: dx_drop rows past the live count were written"
    assert _is_sent16(j["dx"][n:]), f"{tag}: dx rows past the live count were written"
    part = j["part"].cpu()
    assert bool((part != SENT32).all()), f"{tag}: a partial row was not written"
    empty = [b for b in range(n_part) if b * _ln_bwd_waves() >= n]
    if empty:
        assert bool((part[:, empty] == 0).all()), f"{tag}: partials of workgroups without live rows are not zero"
    dg = torch.empty(D, dtype=F32, device="cuda")
    db = torch.empty(D, dtype=F32, device="cuda")
    pkg.ops.colsum_partials([(j["part"], dg, db)], n_part, D, scale)
    errs["dgamma"] = _check_sum(f"{tag} dgamma", dg, scale * (dy[:n] * xh).sum(0), abs(scale) * (dy[:n] * xh).abs().sum(0))
    errs["dbeta"] = _check_sum(f"{tag} dbeta", db, scale * dy[:n].sum(0), abs(scale) * dy[:n].abs().sum(0))
    return errs


LN_BWD_DS = tuple(d for d in LN_DS if d <= 2048)


@DTYPES
@pytest.mark.parametrize("D", LN_BWD_DS, ids=[f"D{d}" for d in LN_BWD_DS])
def test_ln_backward(pkg, D, T16):
    g = torch.Generator().manual_seed(1000 + D)
    eps = LN_EPS[LN_BWD_DS.index(D) % 3]
    R = 4099 if D <= 1024 else 1025
    cases = (   # (rows, n_part, dx_add, dx_drop, drop_rows, live, colsum scale)
        (R, 64, True, True, True, None, 1.0 / GSCALE),
        (9, 1, False, False, False, None, 3.0),
        (9, 3, True, True, False, None, 0.5),
        (7, 16, False, False, False, None, -2.0),
        (197, 8, False, True, True, 150, 1.0),
    )
    for rows, n_part, add, drop, drop_rows, live, scale in cases:
        errs = _ln_bwd_case(pkg, T16, D, rows, n_part, g, eps, add=add, drop=drop, drop_rows=drop_rows, live=live, scale=scale)
        flags = "".join(s for s, on in ((" add", add), (" drop", drop), (" drop_rows", drop_rows)) if on)
        _log(f"ln_backward D={D} rows={rows} live={live if live is not None else rows} n_part={n_part} eps={eps:g}{flags} "
             f"{_name(T16)}", errs)


@DTYPES
@pytest.mark.parametrize("D", [520, 768], ids=["D520", "D768"])
def test_ln_grouped_forward(pkg, D, T16):
    g = torch.Generator().manual_seed(D + 5)
    specs = [(197, 1e-12, None), (4099, 1e-6, 2000), (9, 1e-5, 9), (64, 1e-6, 0)]     # (rows, eps, rows_dev)
    jobs, singles, host = [], [], []
    for rows, eps, live in specs:
        x, kinds = _ln_input(rows, D, g, T16)
        gamma, beta = _ln_params(D, g)
        base = dict(x=_dev(x, T16), gamma=gamma.to(F32).cuda(), beta=beta.to(F32).cuda(), rows=rows, eps=eps,
                    rows_dev=None if live is None else _rows_dev(live))
        jobs.append(dict(base))
        singles.append(dict(base))
        host.append((x, kinds, gamma, beta, eps, rows if live is None else live))
    _ln_fwd_launch(pkg, T16, D, jobs)
    for s in singles:
        _ln_fwd_launch(pkg, T16, D, [s])
    errs = {}
    for i, (j, s, (x, kinds, gamma, beta, eps, n)) in enumerate(zip(jobs, singles, host)):
        for k in ("y", "y32", "mean", "rstd"):
            assert _same_bits(j[k], s[k]), f"job {i}: grouped {k} differs from the single-job launch"
        e = _check_ln_forward(f"ln grouped fwd job {i}", T16, x, kinds, gamma, beta, eps, j, n)
        errs[f"job{i}_y"] = e["y"]
        errs[f"job{i}_rstd"] = e["rstd"]
    _log(f"ln_grouped_fwd D={D} {len(jobs)} jobs {_name(T16)}", errs)


@DTYPES
@pytest.mark.parametrize("D", [520, 768], ids=["D520", "D768"])
def test_ln_grouped_backward(pkg, D, T16):
    g = torch.Generator().manual_seed(D + 9)
    specs = [   # (rows, eps, live, dx_add, drop, drop_rows, n_part): job 0 carries dropout, job 1 does not -- one DROP launch
        (394, 1e-12, 300, False, True, True, 16),
        (197, 1e-6, None, True, False, False, 64),
        (64, 1e-5, 0, True, False, False, 3),
        (129, 1e-6, 129, False, True, False, 5),
    ]
    jobs, singles = [], []
    for rows, eps, live, add, drop, drop_rows, n_part in specs:
        x, _ = _ln_input(rows, D, g, T16, ("randn", "r10", "outlier"))
        gamma, _ = _ln_params(D, g)
        mu, rs = _ln_stats(x, eps)
        base = dict(dy=_dev(_rand((rows, D), g), T16), x=_dev(x, T16), gamma=gamma.to(F32).cuda(), mean=mu.to(F32).cuda(),
                    rstd=rs.to(F32).cuda(), dx_add=_dev(_rand((rows, D), g), T16) if add else None, n_part=n_part, rows=rows,
                    drop=(_rng(5, 2), 0.1, 31) if drop else None, rows_dev=None if live is None else _rows_dev(live),
                    drop_rows=torch.sort(torch.randperm(2 * rows, generator=g)[:rows]).values.to(I32).cuda() if drop_rows else None)
        jobs.append(dict(base))
        singles.append(dict(base))
    _ln_bwd_launch(pkg, T16, D, jobs)
    for s in singles:
        _ln_bwd_launch(pkg, T16, D, [s])
    for i, (j, s, spec) in enumerate(zip(jobs, singles, specs)):
        for k in ("dx", "part", "dx_drop"):
            if k in j:
                assert _same_bits(j[k], s[k]), f"job {i}: grouped {k} differs from the single-job launch"
        n = spec[0] if spec[2] is None else spec[2]
        assert _is_sent16(j["dx"][n:]), f"job {i}: dx rows past the live count were written"
        if "dx_drop" in j:
            assert _is_sent16(j["dx_drop"][n:]), f"job {i}: dx_drop rows past the live count were written"
        empty = [b for b in range(spec[6]) if b * _ln_bwd_waves() >= n]
        if empty:
            assert bool((j["part"][:, empty] == 0).all()), f"job {i}: partials of workgroups without live rows are not zero"
    # the grouped dropout job against float64 too (its single launch is bit-identical, the reference is independent)
    errs = _ln_bwd_case(pkg, T16, D, 394, 16, g, 1e-12, drop=True, drop_rows=True, live=300, scale=0.25,
                        kinds=("randn", "r10", "outlier"))
    _log(f"ln_grouped_bwd D={D} {len(jobs)} jobs {_name(T16)}", errs)


VARIANTS = {
    "rpw4": ({"MEMEHIP_LN_FWD_RPW": "4"}, "test_ln_forward and (D8 or D520 or D1024) or test_ln_grouped_forward and D768"),
    "bwd_waves8": ({"MEMEHIP_LN_BWD_WAVES": "8"}, "test_ln_backward and (D64 or D520 or D1032 or D2048) or test_ln_grouped_backward"),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ln_env_variants(pkg, variant):
    """The variant is chosen from the environment once per process: a subset of the cases above in a fresh child process."""
    env_add, expr = VARIANTS[variant]
    env = dict(os.environ)
    env.update(env_add)
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-k", expr, "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, f"{variant}: child run failed (exit {r.returncode}):\n{tail}"
    passed = [ln for ln in r.stdout.splitlines() if " passed" in ln]
    assert passed and "skipped" not in passed[-1], tail
    parity_log(f"[layer ln_env_variants {variant}] child process: {passed[-1].strip()}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. embeddings and token assembly
# ---------------------------------------------------------------------------------------------------------------------

PAD, CLS, SEP = 0, 101, 102
EMB_FWD = {     # name: (B, S, D, vocab, type0, dropout)
    "D128": (32, 128, 128, 30522, True, False),
    "D768_S512": (2, 512, 768, 30522, True, True),
    "D1024": (4, 200, 1024, 5000, False, True),
    "D4096": (2, 64, 4096, 1000, True, False),
}


def _ids(B, S, V, g):
    """[CLS] tokens [SEP] PAD..., a random length per row; tokens from a narrow range so that ids repeat.  A vocabulary too
    small for the BERT specials (V <= 103) draws every token from [1, V) instead, so that most ids repeat many times."""
    ids = torch.full((B, S), PAD, dtype=I64)
    for b in range(B):
        L = int(torch.randint(max(3, S // 3), S + 1, (1,), generator=g))
        if V <= 103:
            ids[b, :L] = torch.randint(1, V, (L,), generator=g)
            continue
        ids[b, 0] = CLS
        ids[b, 1:L - 1] = torch.randint(103, min(V, 103 + 4 * S), (L - 2,), generator=g)
        ids[b, L - 1] = SEP
    return ids


@DTYPES
@pytest.mark.parametrize("case", list(EMB_FWD))
def test_bert_embed_forward(pkg, case, T16):
    B, S, D, V, has_type, has_drop = EMB_FWD[case]
    g = torch.Generator().manual_seed(D + S)
    eps = 1e-12
    ids = _ids(B, S, V, g)
    P = S + 8         # position table longer than S
    word = (0.05 * _rand((V, D), g)).to(F32)
    pos = (0.02 * _rand((P, D), g)).to(F32)
    type0 = (0.02 * _rand((D,), g)).to(F32) if has_type else None
    gamma, beta = _ln_params(D, g)
    T = B * S
    pre, y = _sent16((T, D), T16), _sent16((T, D), T16)
    mean = torch.full((T,), SENT32, dtype=F32, device="cuda")
    rstd = torch.full((T,), SENT32, dtype=F32, device="cuda")
    drop = (_rng(11, 4), 0.1, 3) if has_drop else None
    pkg.ops.bert_embed_fwd(ids.cuda(), word.cuda(), pos.cuda(), None if type0 is None else type0.cuda(), gamma.to(F32).cuda(),
                           beta.to(F32).cuda(), eps, pre, y, mean, rstd, drop=drop)
    torch.cuda.synchronize()
    w64 = word.to(F64)[ids.flatten()]
    p64 = pos.to(F64)[:S].repeat(B, 1)
    v = w64 + p64
    terms = w64.abs() + p64.abs()
    if type0 is not None:
        v = v + type0.to(F64)
        terms = terms + type0.to(F64).abs()
    errs = {"pre": _check16(f"embed {case} pre", pre, v, T16, TOL_SUM * terms)}
    mu, rs = _ln_stats(v, eps)
    m_k, r_k = _cpu(mean), _cpu(rstd)
    errs["mean"] = _check_sum(f"embed {case} mean", mean, mu, v.abs().mean(1))
    rel = float(((r_k - rs).abs() / rs).max())
    assert rel <= _eps(T16) / 2, f"embed {case} rstd: relative error {rel:.3g} > EPS/2"
    errs["rstd"] = rel / (_eps(T16) / 2)
    d = v - m_k[:, None]
    yv = d * r_k[:, None] * gamma + beta
    yterms = (d.abs() + terms) * r_k[:, None] * gamma.abs() + beta.abs()      # the kernel's sum v carries f32 rounding
    if drop is not None:
        mk = _mask(pkg, T * D, drop).view(T, D) * _drop_scale(drop[1])
        assert 0.85 < float((mk > 0).to(F64).mean()) < 0.95
        yv, yterms = yv * mk, yterms * mk
    errs["y"] = _check16(f"embed {case} y", y, yv, T16, TOL_SUM * yterms)
    _log(f"bert_embed_fwd {case} B={B} S={S} V={V} type0={int(has_type)} drop={int(has_drop)} {_name(T16)}", errs)


EMB_BWD = {     # name: (B, S, D, vocab)
    "prod": (32, 128, 768, 30522),
    "small": (3, 40, 136, 97),
}


@DTYPES
@pytest.mark.parametrize("kernel", ["owner", "indexed"])
@pytest.mark.parametrize("size", list(EMB_BWD))
def test_bert_embed_backward(pkg, size, kernel, T16):
    B, S, D, V = EMB_BWD[size]
    g = torch.Generator().manual_seed(D + V)
    ids = _ids(B, S, V, g)
    T = B * S
    d = _r16(_rand((T, D), g, 4.0), T16)
    scale = 0.37
    dword = torch.zeros((V, D), dtype=F32, device="cuda")
    dpos = torch.full((S + 4, D), SENT32, dtype=F32, device="cuda")
    dtype0 = torch.full((D,), SENT32, dtype=F32, device="cuda")
    row_live = torch.zeros(V, dtype=torch.uint8, device="cuda")
    index = None
    if kernel == "indexed":
        index = (torch.full((V,), 2 ** 31 - 1, dtype=I32, device="cuda"), torch.zeros(V, dtype=I32, device="cuda"))
    pkg.ops.bert_embed_bwd(ids.cuda(), _dev(d, T16), dword, dpos, dtype0, PAD, scale=scale, row_live=row_live, index=index)
    torch.cuda.synchronize()
    flat = ids.flatten()
    keep = flat != PAD
    ref = torch.zeros((V, D), dtype=F64).index_add_(0, flat[keep], d[keep]) * scale
    terms = torch.zeros((V, D), dtype=F64).index_add_(0, flat[keep], d[keep].abs()) * scale
    errs = {"dword": _check_sum(f"embed bwd {size} dword", dword, ref, terms)}
    assert bool((dword[PAD] == 0).all()), "the PAD row received a gradient"
    touched = torch.zeros(V, dtype=torch.bool)
    touched[flat[keep]] = True
    assert torch.equal(row_live.cpu().bool(), touched), "row_live does not mark exactly the rows with a gradient"
    db = d.view(B, S, D)
    errs["dpos"] = _check_sum(f"embed bwd {size} dpos", dpos[:S], scale * db.sum(0), scale * db.abs().sum(0))
    assert bool((dpos[S:] == SENT32).all()), "dpos rows past S were written"
    errs["dtype0"] = _check_sum(f"embed bwd {size} dtype0", dtype0, scale * d.sum(0), scale * d.abs().sum(0))
    if index is not None:
        assert bool((index[0] == 2 ** 31 - 1).all()) and bool((index[1] == 0).all()), "the id index was not restored"
    _log(f"bert_embed_bwd {size} {kernel} B={B} S={S} D={D} V={V} {_name(T16)}", errs)


@DTYPES
@pytest.mark.parametrize("shape", [(32, 196, 768), (8, 576, 1024)], ids=["Np196_D768", "Np576_D1024"])
def test_vit_assemble(pkg, shape, T16):
    B, Np, D = shape
    g = torch.Generator().manual_seed(Np)
    proj = _r16(_rand((B * Np, D), g), T16)
    cls = (0.02 * _rand((D,), g)).to(F32)
    pos = (0.02 * _rand((Np + 1, D), g)).to(F32)
    x = _sent16((B * (Np + 1) + 2, D), T16)
    pkg.ops.vit_assemble_fwd(_dev(proj, T16), cls.cuda(), pos.cuda(), x, B, Np, D)
    torch.cuda.synchronize()
    p64 = pos.to(F64)
    ref = torch.empty((B, Np + 1, D), dtype=F64)
    ref[:, 0] = cls.to(F64) + p64[0]
    ref[:, 1:] = proj.view(B, Np, D) + p64[1:]
    terms = torch.empty_like(ref)
    terms[:, 0] = cls.to(F64).abs() + p64[0].abs()
    terms[:, 1:] = proj.view(B, Np, D).abs() + p64[1:].abs()
    errs = {"x": _check16("vit x", x[:B * (Np + 1)].view(B, Np + 1, D), ref, T16, TOL_SUM * terms)}
    assert _is_sent16(x[B * (Np + 1):]), "rows past B * (Np + 1) were written"
    scale = 1.0 / 3.0
    dx = _r16(_rand((B, Np + 1, D), g, 8.0), T16)
    dproj = _sent16((B * Np + 2, D), T16)
    dcls = torch.full((D,), SENT32, dtype=F32, device="cuda")
    dpos = torch.full((Np + 3, D), SENT32, dtype=F32, device="cuda")
    pkg.ops.vit_assemble_bwd(_dev(dx, T16), dproj, dcls, dpos, B, Np, D, scale=scale)
    torch.cuda.synchronize()
    assert _same_bits(dproj[:B * Np].cpu(), dx[:, 1:].reshape(B * Np, D).to(T16)), "dproj is not dx[:, 1:] bit for bit"
    assert _is_sent16(dproj[B * Np:]), "dproj rows past B * Np were written"
    errs["dpos"] = _check_sum("vit dpos", dpos[:Np + 1], scale * dx.sum(0), scale * dx.abs().sum(0))
    assert bool((dpos[Np + 1:] == SENT32).all()), "dpos rows past Np + 1 were written"
    errs["dcls"] = _check_sum("vit dcls", dcls, scale * dx[:, 0].sum(0), scale * dx[:, 0].abs().sum(0))
    assert torch.equal(dcls.cpu(), dpos[0].cpu()), "dcls != dpos[0]"
    _log(f"vit_assemble B={B} Np={Np} D={D} scale=1/3 {_name(T16)}", errs)
