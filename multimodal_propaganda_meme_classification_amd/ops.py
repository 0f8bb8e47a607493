"""Tensor-level wrappers over the memehip C ABI (one call = one fused HIP op).

PyTorch here is plumbing only: it owns device memory and the current stream.
Every wrapper validates device / dtype / contiguity on the host (a kernel that
faults can reset the GPU), then enqueues on ``torch.cuda.current_stream()``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import (MH_GEMM_ACCUM, MH_GEMM_DERIV_AUX, MH_GEMM_GELU, MH_GEMM_OUT_F32, MH_GEMM_QUICK_GELU, MhColsumJob, MhGemmProblem, MhHeadGrads,
                   MhHeadParams, check)

BF16, F16, F32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int64
H16 = (BF16, F16)          # the two 16-bit storage types; the tensor dtype selects the library build


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _kind(t: torch.Tensor) -> str:
    return "fp16" if t.dtype == F16 else "bf16"


def _L(t: torch.Tensor):
    kind = _kind(t)
    return _lib.load(kind)


def _chk(t: torch.Tensor, dtype, name: str, contiguous: bool = True):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise _lib.MemehipError(f"{name}: memehip kernels need a HIP device tensor (got {t.device}); no CPU fallback")
    if dtype is BF16:                      # "the 16-bit storage type": bf16 or fp16
        if t.dtype not in H16:
            raise TypeError(f"{name}: expected bfloat16/float16, got {t.dtype}")
    elif t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


# ---------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------

class Gemm:
    """One problem of a grouped launch (see MhGemmProblem in include/memehip.h)."""

    __slots__ = ("A", "B", "C", "bias", "residual", "aux", "mul", "rowsum", "M", "N", "K", "lda", "ldb", "ldc",
                 "flags", "alpha", "drop", "rows_dev", "drop_rows", "ksplit")

    def __init__(self, A, B, C, M, N, K, lda, ldb, ldc, bias=None, residual=None, aux=None, mul=None,
                 rowsum=None, gelu=False, accum=False, alpha=1.0, drop=None, rows_dev=None, drop_rows=None, quick=False, ksplit=0,
                 deriv_aux=False):
        self.alpha = alpha
        self.ksplit = int(ksplit)      # > 1: split-K, C holds [ksplit][M][ldc] f32 slabs (see MhGemmProblem.ksplit)
        self.rows_dev, self.drop_rows = rows_dev, drop_rows     # packed token rows: device int32 [1] / int32 [M]
        self.drop = drop            # (rng u32[4] device tensor, p, site id) or None
        self.A, self.B, self.C = A, B, C
        self.bias, self.residual, self.aux, self.mul, self.rowsum = bias, residual, aux, mul, rowsum
        self.M, self.N, self.K, self.lda, self.ldb, self.ldc = M, N, K, lda, ldb, ldc
        self.flags = (MH_GEMM_GELU if gelu else 0) | (MH_GEMM_OUT_F32 if C.dtype == F32 else 0) | \
                     (MH_GEMM_ACCUM if accum else 0) | (MH_GEMM_QUICK_GELU if quick else 0) | (MH_GEMM_DERIV_AUX if deriv_aux else 0)


def _rng(t: Optional[torch.Tensor]):
    """device int32/uint32[4] rng words {seed_lo, seed_hi, step, -} of a dropout site, or None (dropout off)"""
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.int32 and t.numel() >= 4):
        raise TypeError("rng must be a device int32 tensor with 4 words")
    return t.data_ptr()


def _drop(drop):
    return (None, 0.0, 0) if drop is None else (_rng(drop[0]), float(drop[1]), int(drop[2]))


def dropout_mask(n: int, drop, device) -> torch.Tensor:
    """0/1 mask (uint8) the kernels use for element indices 0..n-1 of dropout site `drop` = (rng, p, site)."""
    out = torch.empty(n, dtype=torch.uint8, device=device)
    r, p, sid = _drop(drop)
    check(_lib.load().mh_dropout_mask_u8(_p(out), n, r, p, sid, _stream()), "mh_dropout_mask_u8")
    return out


def dropout_apply(x, drop):
    _chk(x, BF16, "x")
    r, p, sid = _drop(drop)
    check(_L(x).mh_dropout_apply(_p(x), x.numel(), r, p, sid, _stream()), "mh_dropout_apply")
    return x


def _min_elems(rows: int, ld: int, cols: int) -> int:
    return (rows - 1) * ld + cols


def gemm_grouped(problems: Sequence[Gemm], a_kmajor: bool, b_kmajor: bool):
    n = len(problems)
    arr = (MhGemmProblem * n)()
    for i, g in enumerate(problems):
        _chk(g.A, BF16, "A", False), _chk(g.B, BF16, "B", False)
        if g.C.dtype not in (BF16, F16, F32) or not g.C.is_cuda:
            raise TypeError("C must be a 16-bit or f32 device tensor")
        if g.A.dtype != g.B.dtype or (g.C.dtype != F32 and g.C.dtype != g.A.dtype):
            raise TypeError("A, B (and a 16-bit C) must share one 16-bit dtype")
        # extents the kernel will touch
        a_need = _min_elems(g.K, g.lda, g.M) if a_kmajor else _min_elems(g.M, g.lda, g.K)
        b_need = _min_elems(g.K, g.ldb, g.N) if b_kmajor else _min_elems(g.N, g.ldb, g.K)
        c_need = _min_elems(g.M, g.ldc, g.N)
        if g.ksplit > 1:
            c_need = (g.ksplit - 1) * g.M * g.ldc + c_need        # [ksplit][M][ldc] f32 slabs
            if g.C.dtype != F32:
                raise TypeError("split-K needs an f32 output")
        if g.A.numel() < a_need or g.B.numel() < b_need or g.C.numel() < c_need:
            raise ValueError(f"gemm problem {i}: operand smaller than M/N/K/ld imply")
        for nm, t, dt, need in (("bias", g.bias, F32, g.N), ("residual", g.residual, BF16, c_need),
                                ("aux", g.aux, BF16, c_need), ("mul", g.mul, BF16, c_need),
                                ("rowsum", g.rowsum, F32, g.M)):
            if t is not None:
                _chk(t, dt, nm, False)
                if t.numel() < need:
                    raise ValueError(f"gemm problem {i}: {nm} too small")
        a = arr[i]
        a.A, a.B, a.C = _p(g.A), _p(g.B), _p(g.C)
        a.bias, a.residual, a.aux, a.mul, a.rowsum = _p(g.bias), _p(g.residual), _p(g.aux), _p(g.mul), _p(g.rowsum)
        a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.flags, a.alpha = g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.flags, g.alpha
        if g.drop is not None:
            a.drop_rng, a.drop_p, a.drop_stream = _rng(g.drop[0]), float(g.drop[1]), int(g.drop[2])
            a.drop_rows = _p(g.drop_rows)
        if g.rows_dev is not None:
            if not (g.rows_dev.is_cuda and g.rows_dev.dtype == torch.int32):
                raise TypeError("rows_dev must be a device int32 tensor")
            a.rows_dev = _p(g.rows_dev)
        a.ksplit = g.ksplit
    check(_L(problems[0].A).mh_gemm_bf16_grouped(arr, n, int(a_kmajor), int(b_kmajor), _stream()), "mh_gemm_bf16_grouped")


def wgrad_slabs(dy, x, M, N, K, lda, ldb, alpha=1.0, target_tiles: int = 512, max_split: int = 64):
    """The split-K weight-gradient GEMM of wgrad_splitk WITHOUT the slab sum: returns (slabs f32 [nsplit][M][N], nsplit); the
    caller sums the slabs in order (mh_conv_wgrad_finish_batched does it for every convolution of a tower in one launch)."""
    lib = _L(dy)
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    # (target_tiles, ResNet-50 step, ms: 1024 tiles 8.80, 512 8.68, 256 8.69, 128 9.10 -- the slabs are HBM traffic too)
    want = max(1, min(max_split, -(-target_tiles // tiles), K // 256))
    sp = max(1, lib.mh_gemm_ksplit_for(int(K), int(want)))
    slabs = torch.empty((sp, M, N), dtype=F32, device=dy.device)
    gemm_grouped([Gemm(dy, x, slabs, M, N, K, lda, ldb, N, alpha=alpha, ksplit=(sp if sp > 1 else 0))], True, True)
    return slabs, sp


def wgrad_splitk(dy, x, M, N, K, lda, ldb, alpha=1.0, target_tiles: int = 1024, max_split: int = 64):
    """dW[M][N] (f32) = alpha * dy^T x over a long contraction K with few output tiles (conv weight gradients: K = B*H*W,
    M = Cout, N = kh*kw*Cin): split-K inside the grouped GEMM + a fixed-order sum of the slabs (reproducible, no atomics)."""
    lib = _L(dy)
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    want = max(1, min(max_split, -(-target_tiles // tiles), K // 256))
    sp = lib.mh_gemm_ksplit_for(int(K), int(want))
    out = torch.empty((M, N), dtype=F32, device=dy.device)
    if sp <= 1:
        gemm_grouped([Gemm(dy, x, out, M, N, K, lda, ldb, N, alpha=alpha)], True, True)
        return out
    slabs = torch.empty((sp, M, N), dtype=F32, device=dy.device)
    gemm_grouped([Gemm(dy, x, slabs, M, N, K, lda, ldb, N, alpha=alpha, ksplit=sp)], True, True)
    jobs = (MhColsumJob * 1)()
    jobs[0].part, jobs[0].out0, jobs[0].out1 = _p(slabs), _p(out), None
    check(_lib.load().mh_colsum_partials_f32(jobs, 1, sp, M * N, 1.0, _stream()), "mh_colsum_partials_f32")
    return out


def linear_fwd(x, w, bias=None, out=None, residual=None, aux=None, gelu=False, drop=None, quick=False, deriv_aux=False):
    """y[T,N] = epi(x[T,K] @ w[N,K]^T)"""
    T, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((T, N), dtype=x.dtype, device=x.device)
    gemm_grouped([Gemm(x, w, out, T, N, K, x.stride(0), w.stride(0), out.stride(0), bias=bias, residual=residual,
                       aux=aux, gelu=gelu, drop=drop, quick=quick, deriv_aux=deriv_aux)], False, False)
    return out


def linear_dgrad(dy, w, out=None, mul=None, residual=None, quick=False, deriv_aux=False):
    """dx[T,K] = dy[T,N] @ w[N,K]  (optionally * gelu'(mul), + residual)"""
    T, N = dy.shape
    K = w.shape[1]
    if out is None:
        out = torch.empty((T, K), dtype=dy.dtype, device=dy.device)
    gemm_grouped([Gemm(dy, w, out, T, K, N, dy.stride(0), w.stride(0), out.stride(0), mul=mul, residual=residual,
                       quick=quick, deriv_aux=deriv_aux)], False, True)
    return out


def linear_wgrad(dy, x, dw, dbias=None, accum=False, alpha=1.0):
    """dw[N,K] (f32) = dy[T,N]^T @ x[T,K] ; dbias[N] = colsum(dy)"""
    T, N = dy.shape
    K = x.shape[1]
    gemm_grouped([Gemm(dy, x, dw, N, K, T, dy.stride(0), x.stride(0), dw.stride(0), rowsum=dbias, accum=accum, alpha=alpha)],
                 True, True)
    return dw


# ---------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------

def layernorm_fwd(x, gamma, beta, eps, y=None, mean=None, rstd=None, y_f32=None):
    _chk(x, BF16, "x"), _chk(gamma, F32, "gamma"), _chk(beta, F32, "beta")
    rows, D = x.shape
    y = torch.empty_like(x) if y is None else _chk(y, BF16, "y")
    mean = torch.empty(rows, dtype=F32, device=x.device) if mean is None else mean
    rstd = torch.empty(rows, dtype=F32, device=x.device) if rstd is None else rstd
    if y_f32 is not None:
        _chk(y_f32, F32, "y_f32")
        assert y_f32.numel() >= rows * D
    check(_L(x).mh_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(y_f32), _p(mean), _p(rstd), rows, D,
                                       float(eps), _stream()), "mh_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, part, dx=None, dx_add=None, dx_drop=None, drop=None):
    _chk(dy, BF16, "dy"), _chk(x, BF16, "x"), _chk(gamma, F32, "gamma"), _chk(part, F32, "part")
    rows, D = x.shape
    n_part = part.shape[1]
    assert part.shape == (2, n_part, D) and mean.numel() >= rows and rstd.numel() >= rows
    dx = torch.empty_like(x) if dx is None else _chk(dx, BF16, "dx")
    r, p, sid = _drop(drop)
    check(_L(x).mh_layernorm_bwd(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dx_add), _p(dx), _p(part),
                                 n_part, rows, D, _p(dx_drop), r, p, sid, _stream()), "mh_layernorm_bwd")
    return dx


def colsum_partials(jobs, n_part: int, D: int, scale: float = 1.0):
    """jobs: list of (part[2,n_part,D], out0 or None, out1 or None)"""
    for i in range(0, len(jobs), _lib.MH_COLSUM_MAX_JOBS):
        chunk = jobs[i:i + _lib.MH_COLSUM_MAX_JOBS]
        arr = (MhColsumJob * len(chunk))()
        for j, (part, o0, o1) in enumerate(chunk):
            _chk(part, F32, "part")
            assert part.numel() >= 2 * n_part * D
            for o in (o0, o1):
                if o is not None:
                    _chk(o, F32, "out", False)
                    assert o.numel() >= D
            arr[j].part, arr[j].out0, arr[j].out1 = _p(part), _p(o0), _p(o1)
        check(_lib.load().mh_colsum_partials_f32(arr, len(chunk), n_part, D, float(scale), _stream()), "mh_colsum_partials_f32")


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------

def attn_fwd(qkv, key_mask, B, S, H, out=None, lse=None, drop=None):
    _chk(qkv, BF16, "qkv")
    assert qkv.numel() == B * S * 3 * H * 64
    if key_mask is not None:
        _chk(key_mask, I64, "key_mask")
        assert key_mask.numel() == B * S
    out = torch.empty((B * S, H * 64), dtype=qkv.dtype, device=qkv.device) if out is None else _chk(out, BF16, "out")
    lse = torch.empty((B, H, S), dtype=F32, device=qkv.device) if lse is None else _chk(lse, F32, "lse")
    assert out.numel() == B * S * H * 64 and lse.numel() == B * H * S
    r, p, sid = _drop(drop)
    check(_L(qkv).mh_attn_fwd(_p(qkv), _p(key_mask), _p(out), _p(lse), B, S, H, r, p, sid, _stream()), "mh_attn_fwd")
    return out, lse


def pack_plan(mask, pool_index: int):
    """Row bookkeeping of the padding-free text tower (mh_pack_plan). Returns a dict of device tensors."""
    _chk(mask, I64, "mask")
    B, S = mask.shape
    dev = mask.device
    I32 = torch.int32
    out = dict(cu=torch.empty(B + 1, dtype=I32, device=dev), row_map=torch.empty(B * S, dtype=I32, device=dev),
               inv_map=torch.empty(B * S, dtype=I32, device=dev), pmask=torch.empty(B * S, dtype=I64, device=dev),
               pool_rows=torch.empty(B, dtype=I32, device=dev), n_rows=torch.empty(1, dtype=I32, device=dev))
    check(_lib.load().mh_pack_plan(_p(mask), B, S, int(pool_index), _p(out["cu"]), _p(out["row_map"]), _p(out["inv_map"]),
                                   _p(out["pmask"]), _p(out["pool_rows"]), _p(out["n_rows"]), _stream()), "mh_pack_plan")
    return out


def pack_rows(src, plan, D):
    _chk(src, BF16, "src")
    max_rows = plan["row_map"].numel()
    assert src.numel() == max_rows * D
    dst = torch.zeros_like(src)
    check(_L(src).mh_pack_rows(_p(src), _p(plan["row_map"]), _p(plan["n_rows"]), _p(dst), max_rows, D, _stream()),
          "mh_pack_rows")
    return dst


def unpack_rows(src, plan, D):
    _chk(src, BF16, "src")
    max_rows = plan["inv_map"].numel()
    assert src.numel() == max_rows * D
    dst = torch.empty_like(src)
    check(_L(src).mh_unpack_rows(_p(src), _p(plan["inv_map"]), _p(dst), max_rows, D, _stream()), "mh_unpack_rows")
    return dst


def _rows_jobs(jobs, scatter: bool):
    """jobs: dicts of src, dst and the rows' names -- idx (int32 device tensor, ascending) or stride / offset -- plus, for a
    scatter, an optional rows_dev (int32[1]).  The full side is [rows, D], the compact side [n, D]."""
    assert 1 <= len(jobs) <= _lib.MH_ROWS_MAX_JOBS
    arr = (_lib.MhRowsJob * len(jobs))()
    for e, j in zip(arr, jobs):
        src, dst, idx = _chk(j["src"], BF16, "src"), _chk(j["dst"], BF16, "dst"), j.get("idx")
        assert src.dim() == 2 and dst.dim() == 2 and src.dtype == dst.dtype and src.shape[1] == dst.shape[1]
        full, compact = (dst, src) if scatter else (src, dst)
        n, D = compact.shape
        if idx is not None:
            _chk(idx, torch.int32, "idx")
            assert idx.numel() == n
        e.src, e.dst, e.idx, e.rows_dev = _p(src), _p(dst), _p(idx), _p(j.get("rows_dev") if scatter else None)
        e.n, e.rows, e.D, e.stride, e.offset = n, full.shape[0], D, int(j.get("stride", 0)), int(j.get("offset", 0))
    return arr


def rows_gather(jobs):
    """dst[b] = src[row(b)] for every job, one launch (mh_rows_gather)."""
    arr = _rows_jobs(jobs, False)
    check(_L(jobs[0]["src"]).mh_rows_gather(arr, len(jobs), _stream()), "mh_rows_gather")


def rows_scatter_zero(jobs):
    """dst[row(b)] = src[b], every other row of dst (up to rows_dev) zero, for every job, one launch (mh_rows_scatter_zero)."""
    arr = _rows_jobs(jobs, True)
    check(_L(jobs[0]["src"]).mh_rows_scatter_zero(arr, len(jobs), _stream()), "mh_rows_scatter_zero")


def attn_fwd_packed(qkv, plan, B, S, H, drop=None):
    """qkv: packed rows [B*S (max), 3*H*64]; sequences delimited by plan['cu']."""
    _chk(qkv, BF16, "qkv")
    assert qkv.numel() == B * S * 3 * H * 64
    out = torch.zeros((B * S, H * 64), dtype=qkv.dtype, device=qkv.device)
    lse = torch.zeros((B, H, S), dtype=F32, device=qkv.device)
    r, p, sid = _drop(drop)
    check(_L(qkv).mh_attn_fwd_packed(_p(qkv), _p(plan["pmask"]), _p(out), _p(lse), _p(plan["cu"]), _p(plan["row_map"]),
                                     B, S, H, r, p, sid, _stream()), "mh_attn_fwd_packed")
    return out, lse


def attn_bwd_packed(qkv, plan, out, dout, lse, B, S, H, drop=None):
    _chk(qkv, BF16, "qkv"), _chk(out, BF16, "out"), _chk(dout, BF16, "dout"), _chk(lse, F32, "lse")
    assert qkv.numel() == B * S * 3 * H * 64 and out.numel() == B * S * H * 64 == dout.numel()
    dqkv = torch.zeros_like(qkv)
    delta = torch.empty((B, H, S), dtype=F32, device=qkv.device)
    r, p, sid = _drop(drop)
    check(_L(qkv).mh_attn_bwd_packed(_p(qkv), _p(plan["pmask"]), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv),
                                     _p(plan["cu"]), _p(plan["row_map"]), B, S, H, r, p, sid, _stream()),
          "mh_attn_bwd_packed")
    return dqkv


def attn_grouped(problems, backward: bool = False):
    """mh_attn_fwd_grouped / mh_attn_bwd_grouped.  problems: dicts with tensors qkv, out, lse (+ dout, delta, dqkv for the
    backward), optional key_mask, cu, row_map, drop=(rng, p, site) and ints B, S, H.  Outputs are written in place."""
    from ._lib import MhAttnProblem
    arr = (MhAttnProblem * len(problems))()
    for e, d in zip(arr, problems):
        _chk(d["qkv"], BF16, "qkv"), _chk(d["out"], BF16, "out"), _chk(d["lse"], F32, "lse")
        n = d["B"] * d["S"] * d["H"] * 64
        assert d["qkv"].numel() >= 3 * n and d["out"].numel() >= n and d["lse"].numel() >= d["B"] * d["H"] * d["S"]
        if backward:
            _chk(d["dout"], BF16, "dout"), _chk(d["dqkv"], BF16, "dqkv"), _chk(d["delta"], F32, "delta")
            assert d["dout"].numel() >= n and d["dqkv"].numel() >= 3 * n and d["delta"].numel() >= d["B"] * d["H"] * d["S"]
        for k in ("qkv", "key_mask", "out", "lse", "dout", "delta", "dqkv", "cu", "row_map"):
            setattr(e, k, _p(d.get(k)))
        e.rng, e.drop_p, e.drop_stream = _drop(d.get("drop"))
        e.B, e.S, e.H = d["B"], d["S"], d["H"]
    lib = _L(problems[0]["qkv"])
    fn = lib.mh_attn_bwd_grouped if backward else lib.mh_attn_fwd_grouped
    check(fn(arr, len(problems), _stream()), "mh_attn_bwd_grouped" if backward else "mh_attn_fwd_grouped")


def attn_bwd(qkv, key_mask, out, dout, lse, B, S, H, dqkv=None, delta=None, drop=None):
    _chk(qkv, BF16, "qkv"), _chk(out, BF16, "out"), _chk(dout, BF16, "dout"), _chk(lse, F32, "lse")
    assert qkv.numel() == B * S * 3 * H * 64 and out.numel() == B * S * H * 64 == dout.numel()
    assert lse.numel() == B * H * S
    dqkv = torch.empty_like(qkv) if dqkv is None else _chk(dqkv, BF16, "dqkv")
    delta = torch.empty((B, H, S), dtype=F32, device=qkv.device) if delta is None else _chk(delta, F32, "delta")
    assert dqkv.numel() == qkv.numel() and delta.numel() == B * H * S
    r, p, sid = _drop(drop)
    check(_L(qkv).mh_attn_bwd(_p(qkv), _p(key_mask), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv), B, S, H,
                              r, p, sid, _stream()), "mh_attn_bwd")
    return dqkv


# ---------------------------------------------------------------------------------------------
# embeddings / patches
# ---------------------------------------------------------------------------------------------

def bert_embed_fwd(ids, word, pos, type0, gamma, beta, eps, pre, y, mean, rstd, drop=None):
    _chk(ids, I64, "ids"), _chk(word, F32, "word"), _chk(pos, F32, "pos")
    B, S = ids.shape
    V, D = word.shape
    assert pos.shape[0] >= S and pos.shape[1] == D
    assert pre.numel() >= B * S * D and y.numel() >= B * S * D and mean.numel() >= B * S and rstd.numel() >= B * S
    check(_L(pre).mh_bert_embed_fwd(_p(ids), _p(word), _p(pos), _p(type0), _p(gamma), _p(beta),
                                        _p(_chk(pre, BF16, "pre")), _p(_chk(y, BF16, "y")), _p(mean), _p(rstd), B, S,
                                        D, V, float(eps), *_drop(drop), _stream()), "mh_bert_embed_fwd")


def bert_embed_bwd(ids, d_pre, dword, dpos, dtype0, pad_id: int, scale: float = 1.0, row_live=None, index=None):
    """index = (first_pos int32[V] filled with INT32_MAX, id_count int32[V] zeros) selects the linear-time kernel."""
    _chk(ids, I64, "ids"), _chk(d_pre, BF16, "d_pre"), _chk(dword, F32, "dword"), _chk(dpos, F32, "dpos")
    B, S = ids.shape
    V, D = dword.shape
    assert d_pre.numel() >= B * S * D and dpos.shape[0] >= S
    check(_L(d_pre).mh_bert_embed_bwd(_p(ids), _p(d_pre), _p(dword), _p(dpos), _p(dtype0), B, S, D, V, int(pad_id),
                                      float(scale), _p(row_live), _p(index[0]) if index else None,
                                      _p(index[1]) if index else None, _stream()), "mh_bert_embed_bwd")


def position_ids_from_input_ids(ids, pad_id: int, max_position: int, pos_ids=None, pos_inv=None, kind: str = "bf16"):
    """RoBERTa-family position ids (mh_position_ids_from_input_ids): returns (pos_ids int32 [B, S], pos_inv int32 [B, max_position])."""
    _chk(ids, I64, "ids")
    B, S = ids.shape
    I32 = torch.int32
    pos_ids = torch.empty((B, S), dtype=I32, device=ids.device) if pos_ids is None else _chk(pos_ids, I32, "pos_ids")
    pos_inv = torch.empty((B, max_position), dtype=I32, device=ids.device) if pos_inv is None else _chk(pos_inv, I32, "pos_inv")
    assert pos_ids.numel() >= B * S and pos_inv.numel() >= B * max_position
    check(_lib.load(kind).mh_position_ids_from_input_ids(_p(ids), _p(pos_ids), _p(pos_inv), B, S, int(pad_id), int(max_position),
                                                         _stream()), "mh_position_ids_from_input_ids")
    return pos_ids, pos_inv


def bert_embed_fwd_pos(ids, pos_ids, word, pos, type0, gamma, beta, eps, pre, y, mean, rstd, drop=None):
    """bert_embed_fwd with the position row of token t named by pos_ids[t] (mh_bert_embed_fwd_pos)."""
    _chk(ids, I64, "ids"), _chk(pos_ids, torch.int32, "pos_ids"), _chk(word, F32, "word"), _chk(pos, F32, "pos")
    B, S = ids.shape
    V, D = word.shape
    assert pos_ids.numel() >= B * S and pos.shape[1] == D
    assert pre.numel() >= B * S * D and y.numel() >= B * S * D and mean.numel() >= B * S and rstd.numel() >= B * S
    check(_L(pre).mh_bert_embed_fwd_pos(_p(ids), _p(word), _p(pos), _p(type0), _p(gamma), _p(beta), _p(_chk(pre, BF16, "pre")),
                                        _p(_chk(y, BF16, "y")), _p(mean), _p(rstd), B, S, D, V, float(eps), *_drop(drop),
                                        _p(pos_ids), pos.shape[0], _stream()), "mh_bert_embed_fwd_pos")


def embed_pos_bwd(d_pre, pos_inv, dpos, dtype0=None, scratch=None, scale: float = 1.0):
    """Position-table gradient of a RoBERTa-family tower (mh_embed_pos_bwd): d_pre 16-bit [B*S, D], pos_inv int32 [B, P],
    dpos f32 [P, D] (every row written); dtype0 f32 [D] with scratch f32 [S, D] additionally gives the token-type gradient."""
    _chk(d_pre, BF16, "d_pre"), _chk(pos_inv, torch.int32, "pos_inv"), _chk(dpos, F32, "dpos")
    B, P = pos_inv.shape
    D = dpos.shape[1]
    S = d_pre.numel() // (B * D)
    assert d_pre.numel() == B * S * D and dpos.shape[0] == P
    if dtype0 is not None:
        _chk(dtype0, F32, "dtype0"), _chk(scratch, F32, "scratch")
        assert dtype0.numel() >= D and scratch.numel() >= S * D
    check(_L(d_pre).mh_embed_pos_bwd(_p(d_pre), _p(pos_inv), _p(dpos), _p(dtype0), _p(scratch), B, S, D, P, float(scale),
                                     _stream()), "mh_embed_pos_bwd")


def zero_rows(ids, table):
    _chk(ids, I64, "ids"), _chk(table, F32, "table")
    V, D = table.shape
    check(_lib.load().mh_zero_rows_f32(_p(ids), _p(table), ids.numel(), D, V, _stream()), "mh_zero_rows_f32")


def image_normalize_u8(images_u8, mean, std, out=None):
    """uint8 [B,H,W,3] (device) -> f32 [B,3,H,W] = (x/255 - mean)/std: ToTensor + Normalize on the device."""
    if not (images_u8.is_cuda and images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[-1] == 3
            and images_u8.is_contiguous()):
        raise _lib.MemehipError("image_normalize_u8: expected a contiguous uint8 [B,H,W,3] tensor on the HIP device")
    B, H, W, _ = images_u8.shape
    out = torch.empty((B, 3, H, W), dtype=F32, device=images_u8.device) if out is None else _chk(out, F32, "out")
    m = (C.c_float * 3)(*[float(x) for x in mean])
    sd = (C.c_float * 3)(*[float(x) for x in std])
    check(_lib.load().mh_image_normalize_u8(_p(images_u8), _p(out), B, H, W, m, sd, _stream()), "mh_image_normalize_u8")
    return out


def patchify(image, patch: int, out=None, dtype=BF16, ld=None):
    """ld = None: the fast path (patch % 8 == 0, rows of exactly C*p*p elements); ld >= C*p*p: the generic gather with
    zero-filled padding columns (mh_patchify_ld; CLIP's 14x14 patches, 588 -> 640)."""
    _chk(image, F32, "image")
    B, Cc, H, W = image.shape
    rows, K = B * (H // patch) * (W // patch), Cc * patch * patch
    pitch = K if ld is None else int(ld)
    out = torch.empty((rows, pitch), dtype=dtype, device=image.device) if out is None else _chk(out, BF16, "patches")
    assert out.numel() >= rows * pitch
    if ld is None:
        check(_L(out).mh_patchify(_p(image), _p(out), B, Cc, H, W, patch, _stream()), "mh_patchify")
    else:
        check(_L(out).mh_patchify_ld(_p(image), _p(out), B, Cc, H, W, patch, pitch, _stream()), "mh_patchify_ld")
    return out


def copy2d_words(src, ld_src, dst, ld_dst, rows, cols, pad_to):
    """mh_copy2d_u32: dst[r][c] = src[r][c] (c < cols) or 0 (cols <= c < pad_to), in 32-bit words."""
    for nm, t in (("src", src), ("dst", dst)):
        if not t.is_cuda:
            raise _lib.MemehipError(f"{nm}: memehip kernels need a HIP device tensor; no CPU fallback")
    assert src.element_size() == dst.element_size()
    wpe = 4 // src.element_size()          # elements per word
    assert src.numel() >= ((rows - 1) * ld_src + cols) * wpe and dst.numel() >= ((rows - 1) * ld_dst + pad_to) * wpe
    check(_lib.load().mh_copy2d_u32(_p(src), ld_src, _p(dst), ld_dst, rows, cols, pad_to, _stream()), "mh_copy2d_u32")
    return dst


def dwconv_dgrad(dy, wt, B, H, W, addend=None, dx=None, K: int = 7):
    """mh_dwconv_nhwc_dgrad: dx [B*H*W, C] 16-bit = (addend +) the depthwise K x K input gradient of dy, over the forward's tap-major
    f32 weight image wt [K*K, C]."""
    _chk(dy, BF16, "dy"), _chk(wt, F32, "wt")
    C = dy.shape[-1]
    if dy.numel() != B * H * W * C or wt.numel() != K * K * C:
        raise ValueError("dwconv_dgrad: dy / wt do not have the sizes B, H, W, C, K imply")
    dx = torch.empty_like(dy) if dx is None else _chk(dx, BF16, "dx")
    if addend is not None:
        _chk(addend, BF16, "addend")
    if dx.numel() != dy.numel() or dx.dtype != dy.dtype or (addend is not None and (addend.numel() != dy.numel() or addend.dtype != dy.dtype)):
        raise ValueError("dwconv_dgrad: dx / addend must match dy")
    check(_L(dy).mh_dwconv_nhwc_dgrad(_p(dy), _p(wt), _p(addend), _p(dx), B, H, W, C, K, _stream()), "mh_dwconv_nhwc_dgrad")
    return dx


def dwconv_wgrad_workspace_elems(B, H, W, C, K: int = 7) -> int:
    """f32 elements of mh_dwconv_nhwc_wgrad's slab workspace (0: the shape is refused)"""
    return int(_lib.load().mh_dwconv_wgrad_workspace_elems(B, H, W, C, K))


def dwconv_wgrad(x, dy, dw, dbias, B, H, W, scale: float = 1.0, accum: bool = False, workspace=None, K: int = 7):
    """mh_dwconv_nhwc_wgrad: dw f32 [C, 1, K, K] (torch layout) and dbias f32 [C] (or None) from x, dy [B*H*W, C] 16-bit; `workspace`:
    f32, at least dwconv_wgrad_workspace_elems(...) elements (allocated when None)."""
    _chk(x, BF16, "x"), _chk(dy, BF16, "dy"), _chk(dw, F32, "dw")
    C = x.shape[-1]
    if x.dtype != dy.dtype or x.numel() != B * H * W * C or dy.numel() != x.numel() or dw.numel() != C * K * K:
        raise ValueError("dwconv_wgrad: x / dy / dw do not have the sizes B, H, W, C, K imply")
    if dbias is not None and (_chk(dbias, F32, "dbias").numel() != C):
        raise ValueError("dwconv_wgrad: dbias must hold C elements")
    need = dwconv_wgrad_workspace_elems(B, H, W, C, K)
    if need <= 0:
        raise _lib.MemehipError(f"mh_dwconv_nhwc_wgrad: unsupported shape B={B} H={H} W={W} C={C} K={K}")
    if workspace is None:
        workspace = torch.empty(need, dtype=F32, device=x.device)
    elif _chk(workspace, F32, "workspace").numel() < need:
        raise ValueError(f"dwconv_wgrad: workspace holds {workspace.numel()} elements, {need} needed")
    check(_L(x).mh_dwconv_nhwc_wgrad(_p(x), _p(dy), _p(dw), _p(dbias), _p(workspace), B, H, W, C, K, float(scale), int(accum), _stream()),
          "mh_dwconv_nhwc_wgrad")
    return dw


def layer_scale_bwd(W, b, gamma, dWp, dbp, dgamma, dW=None, db=None, accum: bool = False):
    """mh_layer_scale_bwd over a second Linear with layer_scale folded in: dWp [C, K] / dbp [C] (f32) are the folded layer's gradients;
    dgamma[c] = sum_k W dWp + b dbp, dW = gamma dWp, db = gamma dbp.  dW / db default to dWp / dbp (in place); accum adds into dW, db, dgamma."""
    dW, db = dWp if dW is None else dW, dbp if db is None else db
    for nm, t in (("W", W), ("b", b), ("gamma", gamma), ("dWp", dWp), ("dbp", dbp), ("dW", dW), ("db", db), ("dgamma", dgamma)):
        _chk(t, F32, nm)
    C, K = W.shape
    if any(t.numel() != C * K for t in (dWp, dW)) or any(t.numel() != C for t in (b, gamma, dbp, db, dgamma)):
        raise ValueError("layer_scale_bwd: operand sizes do not match W [C, K]")
    if accum and (dW.data_ptr() == dWp.data_ptr() or db.data_ptr() == dbp.data_ptr()):
        raise ValueError("layer_scale_bwd: accum needs dW / db buffers of their own")
    check(_lib.load().mh_layer_scale_bwd(_p(W), _p(b), _p(gamma), _p(dWp), _p(dbp), _p(dW), _p(db), _p(dgamma), C, K, int(accum), _stream()),
          "mh_layer_scale_bwd")
    return dW, db, dgamma


def vit_assemble_fwd(proj, cls, pos, x, B, Np, D):
    _chk(proj, BF16, "proj"), _chk(cls, F32, "cls"), _chk(pos, F32, "pos"), _chk(x, BF16, "x")
    assert proj.numel() >= B * Np * D and cls.numel() >= D and pos.numel() >= (Np + 1) * D and x.numel() >= B * (Np + 1) * D
    check(_L(x).mh_vit_assemble_fwd(_p(proj), _p(cls), _p(pos), _p(x), B, Np, D, _stream()), "mh_vit_assemble_fwd")


def vit_assemble_bwd(dx, dproj, dcls, dpos, B, Np, D, scale: float = 1.0):
    _chk(dx, BF16, "dx"), _chk(dproj, BF16, "dproj"), _chk(dcls, F32, "dcls"), _chk(dpos, F32, "dpos")
    assert dx.numel() >= B * (Np + 1) * D and dproj.numel() >= B * Np * D and dcls.numel() >= D and dpos.numel() >= (Np + 1) * D
    check(_L(dx).mh_vit_assemble_bwd(_p(dx), _p(dproj), _p(dcls), _p(dpos), B, Np, D, float(scale), _stream()), "mh_vit_assemble_bwd")


# ---------------------------------------------------------------------------------------------
# head / loss / optimizer
# ---------------------------------------------------------------------------------------------

def _head_struct(cls, tensors):
    s = cls()
    for name, t in zip(("Wt", "bt", "Wi", "bi", "Wf", "bf_", "Wo", "bo"), tensors):
        _chk(t, F32, name)
        setattr(s, name, _p(t))
    return s


def head_fwd(params, text_hidden, image_hidden, pool_index, pooled, feat, fused, logits, B, S, Nt, Dt, Di, P, Cn,
             drop=None, text_rows=None):
    hp = _head_struct(MhHeadParams, params)
    _chk(text_hidden, F32, "text_hidden"), _chk(image_hidden, F32, "image_hidden")
    assert text_hidden.numel() >= B * S * Dt and image_hidden.numel() >= B * Nt * Di
    assert pooled.numel() >= B * (Dt + Di) and feat.numel() >= B * 2 * P and fused.numel() >= B * P and logits.numel() >= B * Cn
    assert params[0].numel() == P * Dt and params[2].numel() == P * Di and params[4].numel() == P * 2 * P and params[6].numel() == Cn * P
    check(_lib.load().mh_head_fwd(C.byref(hp), _p(text_hidden), _p(image_hidden), pool_index, _p(pooled), _p(feat),
                                  _p(fused), _p(logits), B, S, Nt, Dt, Di, P, Cn, *_drop(drop), _p(text_rows), _stream()),
          "mh_head_fwd")


def head_bwd(params, grads, dlogits, pooled, feat, fused, dfeat, dfused, d_text_hidden, d_image_hidden, pool_index,
             B, S, Nt, Dt, Di, P, Cn, out_scale: float = 1.0, drop=None, text_rows=None):
    hp = _head_struct(MhHeadParams, params)
    hg = _head_struct(MhHeadGrads, grads)
    for a, b in zip(params, grads):
        assert a.numel() == b.numel()
    _chk(d_text_hidden, BF16, "d_text_hidden"), _chk(d_image_hidden, BF16, "d_image_hidden")
    assert d_text_hidden.numel() >= B * S * Dt and d_image_hidden.numel() >= B * Nt * Di
    assert dfeat.numel() >= B * 2 * P and dfused.numel() >= B * P and dlogits.numel() >= B * Cn
    check(_L(d_text_hidden).mh_head_bwd(C.byref(hp), C.byref(hg), _p(dlogits), _p(pooled), _p(feat), _p(fused), _p(dfeat),
                                        _p(dfused), _p(d_text_hidden), _p(d_image_hidden), pool_index, B, S, Nt, Dt, Di, P,
                                        Cn, float(out_scale), *_drop(drop), _p(text_rows), _stream()), "mh_head_bwd")


def bn1d_fwd(x, gamma, beta, running_mean, running_var, eps: float, momentum: float, training: bool, relu: bool = False):
    """mh_bn1d_fwd on f32 [B,F]. Returns (y, save_mean, save_rstd)."""
    _chk(x, F32, "x")
    B, Fn = x.shape
    y = torch.empty_like(x)
    sm, sr = torch.empty(Fn, device=x.device), torch.empty(Fn, device=x.device)
    check(_lib.load().mh_bn1d_fwd(_p(x), Fn, _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(y), Fn, _p(sm), _p(sr),
                                  B, Fn, float(eps), float(momentum), int(training), int(relu), _stream()), "mh_bn1d_fwd")
    return y, sm, sr


def bn1d_bwd(dy, x, y, gamma, save_mean, save_rstd, relu: bool = False, frozen_stats: bool = False):
    """mh_bn1d_bwd. Returns (dx, dgamma, dbeta).  ``frozen_stats``: the forward ran in eval mode (MH_BN_FROZEN_STATS)."""
    _chk(dy, F32, "dy"), _chk(x, F32, "x")
    B, Fn = x.shape
    dx = torch.empty_like(x)
    dg, db = torch.empty(Fn, device=x.device), torch.empty(Fn, device=x.device)
    check(_lib.load().mh_bn1d_bwd(_p(dy), Fn, _p(x), Fn, _p(y), Fn, _p(gamma), _p(save_mean), _p(save_rstd), _p(dx), Fn, _p(dg),
                                  _p(db), B, Fn, int(relu) | (2 if frozen_stats else 0), _stream()), "mh_bn1d_bwd")
    return dx, dg, db


def ce_fwd_bwd(logits, labels, loss, dlogits, n_correct=None, grad_scale: float = 1.0, grad_scale_dev=None):
    _chk(logits, F32, "logits"), _chk(labels, I64, "labels"), _chk(loss, F32, "loss"), _chk(dlogits, F32, "dlogits")
    B, Cn = logits.shape
    assert labels.numel() >= B and dlogits.numel() >= B * Cn
    if n_correct is not None:
        _chk(n_correct, torch.int32, "n_correct")
    check(_lib.load().mh_ce_fwd_bwd(_p(logits), _p(labels), _p(loss), _p(dlogits), _p(n_correct), B, Cn,
                                    float(grad_scale), _p(grad_scale_dev), _stream()), "mh_ce_fwd_bwd")


def focal_fwd_bwd(logits, targets, loss, dlogits, n_correct=None, alpha=0.25, gamma=2.0, grad_scale=1.0, grad_scale_dev=None):
    """logits f32 [B] or [B,1]; targets f32 [B]"""
    _chk(logits, F32, "logits"), _chk(targets, F32, "targets"), _chk(loss, F32, "loss"), _chk(dlogits, F32, "dlogits")
    B = targets.numel()
    assert logits.numel() == B == dlogits.numel()
    check(_lib.load().mh_focal_fwd_bwd(_p(logits), 1, _p(targets), _p(loss), _p(dlogits), _p(n_correct), B, float(alpha),
                                       float(gamma), float(grad_scale), _p(grad_scale_dev), _stream()), "mh_focal_fwd_bwd")


REDUCTIONS = {"mean": _lib.MH_LOSS_MEAN, "sum": _lib.MH_LOSS_SUM, "none": _lib.MH_LOSS_NONE}


def ce_opts_fwd_bwd(logits, labels, loss, dlogits, n_correct=None, class_weight=None, ignore_index=None, label_smoothing: float = 0.0,
                    reduction: str = "mean", grad_scale: float = 1.0, grad_scale_dev=None):
    """mh_ce_opts_fwd_bwd: F.cross_entropy(weight=, ignore_index=, label_smoothing=, reduction=).  ``ignore_index=None``: no label is
    ignored.  ``loss`` holds 1 value, or B with reduction "none" (dlogits is then each row's own derivative)."""
    _chk(logits, F32, "logits"), _chk(labels, I64, "labels"), _chk(loss, F32, "loss"), _chk(dlogits, F32, "dlogits")
    B, Cn = logits.shape
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    assert labels.numel() >= B and dlogits.numel() >= B * Cn and loss.numel() >= (B if reduction == "none" else 1)
    if n_correct is not None:
        _chk(n_correct, torch.int32, "n_correct")
    if class_weight is not None:
        _chk(class_weight, F32, "class_weight")
        if class_weight.numel() != Cn:
            raise ValueError(f"class_weight has {class_weight.numel()} entries for {Cn} classes")
    check(_lib.load().mh_ce_opts_fwd_bwd(_p(logits), _p(labels), _p(class_weight), _p(loss), _p(dlogits), _p(n_correct), B, Cn,
                                         0 if ignore_index is None else int(ignore_index), int(ignore_index is not None),
                                         float(label_smoothing), REDUCTIONS[reduction], float(grad_scale), _p(grad_scale_dev), _stream()),
          "mh_ce_opts_fwd_bwd")


def bce_fwd_bwd(logits, targets, loss, dlogits, n_correct=None, pos_weight: float = 1.0, reduction: str = "mean", grad_scale=1.0,
                grad_scale_dev=None, ld: int = 1):
    """mh_bce_fwd_bwd: logits f32 [B] or [B,1] (or column 0 of [B, ld]); targets f32 [B]; dlogits laid out like logits."""
    _chk(logits, F32, "logits"), _chk(targets, F32, "targets"), _chk(loss, F32, "loss"), _chk(dlogits, F32, "dlogits")
    B = targets.numel()
    if reduction not in ("mean", "sum"):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    assert ld >= 1 and logits.numel() >= (B - 1) * ld + 1 and dlogits.numel() >= (B - 1) * ld + 1
    if n_correct is not None:
        _chk(n_correct, torch.int32, "n_correct")
    check(_lib.load().mh_bce_fwd_bwd(_p(logits), int(ld), _p(targets), float(pos_weight), _p(loss), _p(dlogits), _p(n_correct), B,
                                     REDUCTIONS[reduction], float(grad_scale), _p(grad_scale_dev), _stream()), "mh_bce_fwd_bwd")


def sumsq(g, workspace, out):
    _chk(g, F32, "g"), _chk(workspace, F32, "workspace"), _chk(out, F32, "out")
    assert workspace.numel() >= 1024
    check(_lib.load().mh_sumsq_f32(_p(g), g.numel(), _p(workspace), _p(out), _stream()), "mh_sumsq_f32")


def adam_step(p, m, v, g, shadow, n_shadow, hyper, decoupled=False, gnorm_sq=None, max_norm=0.0, overflow=None, ordinal=0, clip_norm_mult=0.0):
    for nm, t in (("p", p), ("m", m), ("v", v), ("g", g), ("hyper", hyper)):
        _chk(t, F32, nm)
    n = p.numel()
    assert m.numel() == n and v.numel() == n and g.numel() == n and hyper.numel() >= 8
    if shadow is not None:
        _chk(shadow, BF16, "shadow")
        assert shadow.numel() >= n_shadow
    check(_L(shadow if shadow is not None else p).mh_adam_step(_p(p), _p(m), _p(v), _p(g), _p(shadow), n, n_shadow if shadow is not None else 0,
                                   _p(hyper), int(decoupled), _p(gnorm_sq), float(max_norm), float(clip_norm_mult), _p(overflow), int(ordinal), _stream()), "mh_adam_step")


def adam_step_rows(p, m, v, g, row_live, row_touched, rows, D, hyper, decoupled=False, gnorm_sq=None, max_norm=0.0, overflow=None, ordinal=0, clip_norm_mult=0.0):
    """mh_adam_step_rows: Adam over a [rows][D] table, rows with no gradient history skipped (row_live |= row_touched)."""
    for nm, t in (("p", p), ("m", m), ("v", v), ("g", g), ("hyper", hyper)):
        _chk(t, F32, nm)
    n = rows * D
    assert p.numel() == n and m.numel() == n and v.numel() == n and g.numel() == n and hyper.numel() >= 8
    if not (row_live.is_cuda and row_live.dtype == torch.uint8 and row_live.numel() >= rows):
        raise TypeError("row_live must be a device uint8 tensor with one byte per row")
    check(_lib.load().mh_adam_step_rows(_p(p), _p(m), _p(v), _p(g), _p(row_live), _p(row_touched), rows, D, _p(hyper), int(decoupled),
                                        _p(gnorm_sq), float(max_norm), float(clip_norm_mult), _p(overflow), int(ordinal), _stream()), "mh_adam_step_rows")


def cast_f32_bf16(src, dst):
    _chk(src, F32, "src"), _chk(dst, BF16, "dst")
    assert dst.numel() >= src.numel()
    check(_L(dst).mh_cast_f32_bf16(_p(src), _p(dst), src.numel(), _stream()), "mh_cast_f32_bf16")


def cast_bf16_f32(src, dst):
    """dst f32 [n] = src 16-bit [n]  (mh_cast_bf16_f32)"""
    _chk(src, BF16, "src"), _chk(dst, F32, "dst")
    assert dst.numel() >= src.numel()
    check(_L(src).mh_cast_bf16_f32(_p(src), _p(dst), src.numel(), _stream()), "mh_cast_bf16_f32")


def sum_shards_16(shards, out, W: int):
    """out[i] = 16-bit(sum_w shards[w][i]), fp32 accumulation (mh_sum_shards_16)"""
    _chk(shards, BF16, "shards"), _chk(out, BF16, "out")
    shard = out.numel()
    assert shards.numel() >= W * shard and shards.dtype == out.dtype
    check(_L(out).mh_sum_shards_16(_p(shards), _p(out), int(W), shard, _stream()), "mh_sum_shards_16")


# ---------------------------------------------------------------------------------------------
# autoregressive decode (decode.hip; blip.BlipCaptioner)
# ---------------------------------------------------------------------------------------------

def decode_splits(B: int, H: int, T: int) -> int:
    """Key splits of mh_attn_decode: 1 when the B*H workgroups fill the chip's 256 CUs, else enough chunks of >= 64 keys to
    reach about 256 workgroups (B = 1, H = 12: 12 workgroups -> up to 22 splits of a long cache)."""
    if B * H >= 256:
        return 1
    return max(1, min(64, -(-256 // (B * H)), -(-T // 64)))


def _i32(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32):
        raise _lib.MemehipError(f"{name}: expected a device int32 tensor")
    return t


def attn_decode(q, k, v, out, B, H, T, ldq, ld_b, ld_t, ldo, t_dev=None, kv_new=None, ld_new=0, nsplit=None, workspace=None,
                kv_group=1, src=None):
    """mh_attn_decode: out[b, h] = softmax(q[b, h] . k[b, h, :T]^T / 8) v[b, h, :T] (16-bit views with element strides; see the
    header).  t_dev (device int32 [1]) selects the self-attention form: kv_new's k / v rows are stored into slot t first and keys
    0..t attend (T = the cache capacity).  nsplit None: decode_splits(B, H, T); a workspace is allocated when it is > 1.
    Beams (mh_attn_decode_beams): kv_group rows share the k / v of row b // kv_group; src (device int32 [B, >= T], self form) names
    the cache row that holds key j < t of row b."""
    for nm, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        _chk(t, BF16, nm, False)
    if len({q.dtype, k.dtype, v.dtype, out.dtype}) != 1:
        raise TypeError("attn_decode: q, k, v, out must share one 16-bit dtype")
    if t_dev is not None:
        _i32(t_dev, "t_dev")
        _chk(kv_new, BF16, "kv_new", False)
        if kv_new.dtype != q.dtype or kv_new.numel() < (B - 1) * ld_new + 2 * H * 64:
            raise ValueError("attn_decode: kv_new smaller than B / ld_new / H imply")
    if q.numel() < (B - 1) * ldq + H * 64 or out.numel() < (B - 1) * ldo + H * 64:
        raise ValueError("attn_decode: q / out smaller than B / ld / H imply")
    kv_group = int(kv_group)
    if kv_group < 1 or B % kv_group or (t_dev is not None and kv_group != 1):
        raise ValueError("attn_decode: kv_group must divide B, and be 1 in the self form")
    if src is not None:
        _i32(src, "src")
        if t_dev is None or src.dim() != 2 or src.shape[0] != B or src.shape[1] < T or not src.is_contiguous():
            raise ValueError("attn_decode: src is a contiguous int32 [B, >= T] table of the self form")
    need = (B // kv_group - 1) * ld_b + (T - 1) * ld_t + H * 64
    if k.numel() < need or v.numel() < need:
        raise ValueError("attn_decode: k / v smaller than B / T / strides imply")
    nsplit = decode_splits(B, H, T) if nsplit is None else int(nsplit)
    if nsplit > 1:
        if workspace is None:
            workspace = torch.empty(B * H * nsplit * 66, dtype=F32, device=q.device)
        _chk(workspace, F32, "workspace")
        if workspace.numel() < B * H * nsplit * 66:
            raise ValueError("attn_decode: workspace smaller than B * H * nsplit * 66")
    if kv_group == 1 and src is None:
        check(_L(q).mh_attn_decode(_p(q), int(ldq), _p(k), _p(v), int(ld_b), int(ld_t), _p(kv_new), int(ld_new), _p(t_dev), int(T), _p(out),
                                   int(ldo), _p(workspace) if nsplit > 1 else None, nsplit, int(B), int(H), _stream()), "mh_attn_decode")
    else:
        check(_L(q).mh_attn_decode_beams(_p(q), int(ldq), _p(k), _p(v), int(ld_b), int(ld_t), _p(kv_new), int(ld_new), _p(t_dev), int(T),
                                         _p(out), int(ldo), _p(workspace) if nsplit > 1 else None, nsplit, int(B), int(H), kv_group,
                                         _p(src), src.shape[1] if src is not None else 0, _stream()), "mh_attn_decode_beams")
    return out


def decode_embed(ids, t_dev, word, pos, gamma, beta, eps, y):
    """mh_decode_embed: y[b] = LayerNorm(word[ids[b]] + pos[t]) (16-bit [B, D])."""
    _chk(ids, I64, "ids"), _i32(t_dev, "t_dev"), _chk(word, F32, "word"), _chk(pos, F32, "pos")
    _chk(gamma, F32, "gamma"), _chk(beta, F32, "beta"), _chk(y, BF16, "y")
    B = ids.numel()
    V, D = word.shape
    if pos.shape[1] != D or gamma.numel() != D or beta.numel() != D or y.numel() < B * D:
        raise ValueError("decode_embed: table / output widths disagree")
    check(_L(y).mh_decode_embed(_p(ids), _p(t_dev), _p(word), _p(pos), _p(gamma), _p(beta), _p(y), B, D, V, pos.shape[0], float(eps),
                                _stream()), "mh_decode_embed")
    return y


def logits_process(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0):
    """The settings of greedy_step / beam_step's ``process`` (MhLogitsProcess in include/memehip.h), validated: the penalty a finite
    number > 0, the other three integers >= 0.  The defaults are neutral."""
    import math
    p = repetition_penalty
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not math.isfinite(p) or not p > 0:
        raise ValueError(f"repetition_penalty must be a finite number > 0, got {p!r}")
    ints = dict(no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, min_new_tokens=min_new_tokens)
    for name, v in ints.items():
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 31:
            raise ValueError(f"{name} must be an integer >= 0, got {v!r}")
    return _lib.MhLogitsProcess(float(p), *ints.values())


def process_is_neutral(process) -> bool:
    if process is not None and not isinstance(process, _lib.MhLogitsProcess):
        raise TypeError("process is a logits_process(...) or None")
    return process is None or (process.repetition_penalty == 1.0 and process.no_repeat_ngram_size == 0 and process.min_length == 0
                               and process.min_new_tokens == 0)


def _check_processed(status, what, limits):
    """the processed entry points refuse a shape outside their limits with MH_ESHAPE: a ValueError that names the limits"""
    if status == _lib.MH_ESHAPE:
        raise ValueError(f"{what}: with logits processors {limits}")
    check(status, what)


def greedy_step(logits, V, out_ids, next_ids, finished, state, prompt_len, eos_id, pad_id, process=None):
    """mh_greedy_step over f32 logits [B, ldl] (ldl >= V): see include/memehip.h.  process: a logits_process() (None or neutral
    settings: the plain entry point), applied to the raw logits before the argmax."""
    _chk(logits, F32, "logits"), _chk(out_ids, I64, "out_ids"), _chk(next_ids, I64, "next_ids")
    _i32(finished, "finished"), _i32(state, "state")
    B, ldl = logits.shape
    if out_ids.dim() != 2 or out_ids.shape[0] != B or next_ids.numel() < B or finished.numel() < B or state.numel() < 4 or V > ldl:
        raise ValueError("greedy_step: shapes disagree")
    if process_is_neutral(process):
        check(_lib.load().mh_greedy_step(_p(logits), ldl, int(V), B, _p(out_ids), out_ids.shape[1], _p(next_ids), _p(finished), _p(state),
                                         int(prompt_len), int(eos_id), int(pad_id), _stream()), "mh_greedy_step")
        return
    _check_processed(_lib.load().mh_greedy_step_processed(_p(logits), ldl, int(V), B, _p(out_ids), out_ids.shape[1], _p(next_ids),
                                                          _p(finished), _p(state), int(prompt_len), int(eos_id), int(pad_id),
                                                          C.byref(process), _stream()), "mh_greedy_step_processed",
                     f"V <= {_lib.MH_PROCESS_MAX_VOCAB} and at most {_lib.MH_PROCESS_MAX_HISTORY} output columns are supported "
                     f"(V = {int(V)}, {out_ids.shape[1]} columns)")


def sampling(temperature=1.0, top_k=0, top_p=1.0):
    """The settings of sample_step's ``sampling`` (MhSampling in include/memehip.h), validated: the temperature a finite number > 0,
    top_k an integer >= 0 (0: no top-k filter), top_p a number in (0, 1].  The defaults are neutral: a draw from the whole softmax."""
    import math
    for name, v in (("temperature", temperature), ("top_p", top_p)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if not temperature > 0 or not C.c_float(temperature).value > 0 or math.isinf(C.c_float(temperature).value):
        raise ValueError(f"temperature must be > 0 (and a finite float32), got {temperature!r}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 0 <= top_k < 2 ** 31:
        raise ValueError(f"top_k must be an integer >= 0, got {top_k!r}")
    if not 0 < top_p <= 1 or not C.c_float(top_p).value > 0:
        raise ValueError(f"top_p must lie in (0, 1], got {top_p!r}")
    return _lib.MhSampling(float(temperature), top_k, float(top_p))


def sampling_is_neutral(sampling) -> bool:
    if not isinstance(sampling, _lib.MhSampling):
        raise TypeError("sampling is a sampling(...)")
    return sampling.temperature == 1.0 and sampling.top_k == 0 and sampling.top_p == 1.0


def sample_rng(seed: int, device) -> torch.Tensor:
    """device int32 [4] {seed_lo, seed_hi, 0, 0}: the seed words of sample_step (the low 64 bits of ``seed``)"""
    t = torch.zeros(4, dtype=torch.int32, device=device)
    return set_sample_rng(t, seed)


def set_sample_rng(rng: torch.Tensor, seed: int) -> torch.Tensor:
    """writes the low 64 bits of ``seed`` into rng[0:2] (a buffer a captured step reads keeps its address)"""
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"seed must be an integer, got {seed!r}")
    words = [(seed >> s) & 0xffffffff for s in (0, 32)]
    rng[:2].copy_(torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32))
    return rng


def sample_step(logits, V, out_ids, next_ids, finished, state, prompt_len, eos_id, pad_id, sampling, rng, u_out=None, process=None):
    """mh_sample_step over f32 logits [B, ldl] (ldl >= V): the greedy step with a temperature / top-k / top-p filtered multinomial
    draw in place of the argmax; see include/memehip.h.  sampling: a sampling(); rng: device int32 [4] (sample_rng); u_out: None or
    device f32 [B], receives each row's uniform; process: a logits_process() applied first (None or neutral: none)."""
    _chk(logits, F32, "logits"), _chk(out_ids, I64, "out_ids"), _chk(next_ids, I64, "next_ids")
    _i32(finished, "finished"), _i32(state, "state")
    if not isinstance(sampling, _lib.MhSampling):
        raise TypeError("sampling is a sampling(...)")
    B, ldl = logits.shape
    if out_ids.dim() != 2 or out_ids.shape[0] != B or next_ids.numel() < B or finished.numel() < B or state.numel() < 4 or V > ldl:
        raise ValueError("sample_step: shapes disagree")
    if u_out is not None and (_chk(u_out, F32, "u_out").numel() < B):
        raise ValueError("sample_step: u_out holds fewer than B values")
    neutral = process_is_neutral(process)
    status = _lib.load().mh_sample_step(_p(logits), ldl, int(V), B, _p(out_ids), out_ids.shape[1], _p(next_ids), _p(finished), _p(state),
                                        int(prompt_len), int(eos_id), int(pad_id), C.byref(sampling), _rng(rng), _p(u_out),
                                        None if neutral else C.byref(process), _stream())
    if status == _lib.MH_ESHAPE and int(V) > _lib.MH_PROCESS_MAX_VOCAB:
        raise ValueError(f"mh_sample_step: V <= {_lib.MH_PROCESS_MAX_VOCAB} is supported (V = {int(V)})")
    if neutral:
        check(status, "mh_sample_step")
    else:
        _check_processed(status, "mh_sample_step", f"V <= {_lib.MH_PROCESS_MAX_VOCAB} and at most {_lib.MH_PROCESS_MAX_HISTORY} output "
                         f"columns are supported (V = {int(V)}, {out_ids.shape[1]} columns)")


BEAM_NEG = -1.0e9


def beam_state(B, K, cap, prompt, pad_id, device, src=True):
    """The device state of mh_beam_step for B images of K beams, at its start values (include/memehip.h): a dict of tensors, rows
    [image][beam].  prompt: int [B, P] (every beam of an image starts from it); src: also the cache ancestry table."""
    B, K, cap = int(B), int(K), int(cap)
    prompt = torch.as_tensor(prompt).to(device=device, dtype=torch.int32)
    if prompt.dim() != 2 or prompt.shape[0] != B or not 1 <= prompt.shape[1] < cap:
        raise ValueError("beam_state: prompt must be [B, P] with 1 <= P < cap")
    if not 2 <= K <= 8:
        raise ValueError("beam_state: 2 <= K <= 8")
    R = B * K
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device=device)
    run_seq = torch.full((R, cap), int(pad_id), dtype=torch.int32, device=device)
    run_seq[:, :prompt.shape[1]] = prompt.repeat_interleave(K, 0)
    run_scores = torch.full((B, K), BEAM_NEG, dtype=F32, device=device)
    run_scores[:, 0] = 0.0
    st = dict(B=B, K=K, cap=cap, next_ids=run_seq[:, 0].to(I64).contiguous(), parents=z(R), run_scores=run_scores.view(R), run_seq=run_seq,
              src=torch.arange(R, dtype=torch.int32, device=device).view(R, 1).repeat(1, cap) if src else None,
              fin_seq=run_seq.clone(), fin_scores=torch.full((R,), BEAM_NEG, dtype=F32, device=device), fin_flags=z(R), fin_len=z(R),
              heur=torch.ones(B, dtype=torch.int32, device=device), state=z(4), cand_val=z(R, 2 * K, dt=F32), cand_idx=z(R, 2 * K))
    st["_c"] = _lib.MhBeamState(**{n: _p(st[n]) for n, _ in _lib.MhBeamState._fields_})
    return st


def beam_step(logits, V, st, prompt_len, length_penalty, early_stopping, eos_id, process=None):
    """mh_beam_step over f32 logits [B * K, ldl] (ldl >= V) on a beam_state: see include/memehip.h.  process: a logits_process()
    (None or neutral settings: the plain entry point), applied to each row's log-softmax before its running score is added."""
    _chk(logits, F32, "logits")
    if not isinstance(early_stopping, bool) and early_stopping != "never":
        raise ValueError("beam_step: early_stopping is False, True or 'never'")
    B, K, cap = st["B"], st["K"], st["cap"]
    if logits.dim() != 2 or logits.shape[0] != B * K or not logits.is_contiguous() or V > logits.shape[1]:
        raise ValueError("beam_step: logits must be a contiguous [B * K, ldl >= V]")
    for n, _ in _lib.MhBeamState._fields_:
        if st[n] is not None and getattr(st["_c"], n) != st[n].data_ptr():
            raise ValueError(f"beam_step: state tensor {n!r} was replaced after beam_state()")
    es = 1 if early_stopping is True else (2 if early_stopping == "never" else 0)
    if process_is_neutral(process):
        check(_lib.load().mh_beam_step(_p(logits), logits.shape[1], int(V), B, K, C.byref(st["_c"]), cap, int(prompt_len),
                                       float(length_penalty), es, int(eos_id), _stream()), "mh_beam_step")
        return
    _check_processed(_lib.load().mh_beam_step_processed(_p(logits), logits.shape[1], int(V), B, K, C.byref(st["_c"]), cap, int(prompt_len),
                                                        float(length_penalty), es, int(eos_id), C.byref(process), _stream()),
                     "mh_beam_step_processed",
                     f"2K + cap + 1 <= V <= {_lib.MH_PROCESS_MAX_VOCAB} and cap <= {_lib.MH_PROCESS_MAX_HISTORY} are needed "
                     f"(V = {int(V)}, K = {K}, cap = {cap}: every row must keep 2K candidates that are not banned)")


# ---------------------------------------------------------------------------------------------
# SVM (svm.hip): the batched C-SVC solver.  svm.py drives these two.
# ---------------------------------------------------------------------------------------------

F64 = torch.float64


def _svc_problem(K, y, Cv, alpha, G, state, tol, budget, max_iter):
    """MhSvcProblem over K f32 [n, ldk], y f32 [n], Cv / alpha / G f64 [P, n], state f64 [P, MH_SVC_STATE]; shapes checked here,
    the limits (n <= MH_SVC_MAX_N, P <= MH_SVC_MAX_PROBLEMS) by the library."""
    _chk(K, F32, "K"), _chk(y, F32, "y")
    for name, t in (("Cv", Cv), ("alpha", alpha), ("G", G), ("state", state)):
        _chk(t, F64, name)
    if Cv.dim() != 2 or K.dim() != 2:
        raise ValueError("svc: K is [n, ldk] and Cv is [P, n]")
    P, n = Cv.shape
    if K.shape[0] != n or K.shape[1] < n or y.numel() != n or alpha.shape != Cv.shape or G.shape != Cv.shape or \
            tuple(state.shape) != (P, _lib.MH_SVC_STATE):
        raise ValueError("svc: K [n, ldk >= n], y [n], Cv / alpha / G [P, n] and state [P, MH_SVC_STATE] do not fit together")
    p = _lib.MhSvcProblem()
    p.K, p.y, p.Cv, p.alpha, p.G, p.state = _p(K), _p(y), _p(Cv), _p(alpha), _p(G), _p(state)
    p.n, p.ldk, p.P, p.budget, p.max_iter, p.tol = n, K.shape[1], P, int(budget), int(max_iter), float(tol)
    return p


def svc_init(K, y, Cv, alpha, G, state):
    """mh_svc_init: alpha = 0, G = -1, every problem MH_SVC_RUNNING with 0 iterations."""
    p = _svc_problem(K, y, Cv, alpha, G, state, 1e-3, 1, -1)
    check(_lib.load().mh_svc_init(C.byref(p), _stream()), "mh_svc_init")


def svc_solve(K, y, Cv, alpha, G, state, tol: float = 1e-3, budget: int = _lib.MH_SVC_LAUNCH_ITERS, max_iter: int = -1):
    """mh_svc_solve: ONE launch of at most ``budget`` SMO iterations per problem; alpha, G and state carry on from where they are.
    state[p] = {status, iterations so far, gap, rho}: launch again while a status is MH_SVC_RUNNING (svm.solve_batch does)."""
    p = _svc_problem(K, y, Cv, alpha, G, state, tol, budget, max_iter)
    check(_lib.load().mh_svc_solve(C.byref(p), _stream()), "mh_svc_solve")
