"""The ConvNeXt kernels and launch plan (csrc/dwconv.hip, convnext.py) and the layout kernels (csrc/conv.hip, csrc/embed.hip)
against one plain reference: float64 torch on the CPU, computed from the same 16-bit (or f32) tensors the kernels read, rounded
to 16 bits exactly where a kernel stores 16 bits.

  case                                   kernel / path
  ----------------------------------------------------------------------------------------------------------------------------
  dwconv C<c>                            dwconv_kernel<7, 7> (H and W multiples of 7, not of 8) and <8, 7>, N(0, 1) data,
                                           H x W in {1x1 7x7 8x8 9x13 14x21 28x28 56x56 1x64}, C in {8 96 192 200 384 768} (every
                                           channel-chunk branch: 96 / 192 / 40 channels), with and without bias
  cnblock d<d> <hxw>                     one CNBlock of convnext.py at each stage width, at its 224-image size and a ragged size:
                                           dwconv -> LayerNorm -> GEMM + GELU -> GEMM + bias + residual (layer scale folded as
                                           _packed folds it; d = 96 through the K = 128 re-pitched rows), from the kernel's stem
  stem / downsample d<d>                 mh_patchify_ld + GEMM + LayerNorm; LayerNorm + 2x2 mh_im2col_nhwc + GEMM
  tower <hxw> B<b>                       pooled_features at 32x32, 64x96, 96x64, 224x320 against oracle/convnext_oracle.py, and the
                                           classifier (ConvNeXtTiny.forward: LayerNorm + Linear, from the kernel's pooled features)
  batch independence                     an Inf / NaN pixel in one image leaves every other image's pooled features finite and
                                           bit-identical to a run without it
  layout <kernel>                        bit-exact: mh_nchw_to_nhwc, mh_conv_weight_pack / _unpack / _pack_batched (ResNet-50's 53
                                           convolutions), mh_patchify (P 8 16 32), mh_patchify_ld (P 1 4 14 16), mh_copy2d_u32,
                                           mh_zero_rows_f32, mh_image_normalize_u8

Bars (TOL_SUM = 1e-5, EPS32 = 2^-24, ulp = the 16-bit ulp; every bound is per element):
  * a stored sum (dwconv, GEMM + epilogue): |hip - ref| <= 1 ulp + TOL_SUM x sum|terms| (f32 accumulation), plus the propagated
    error of its inputs: sum_k |w_k| e_k for a linear map with input bounds e_k;
  * an input of a later stage differs from the reference's rounded value by its own bound plus 1 ulp (the reference and the
    kernel may round to neighbouring 16-bit values);
  * LayerNorm: input errors e map through |gamma| rstd (e + mean(e) + |yhat| mean(|yhat| e)) (the first-order change of
    (t - mean) rstd); its own f32 statistics add |gamma| rstd (dm + |t - mean| dr) with dm = TOL_SUM sum|t| / D, dr = (TOL_SUM +
    (dm / std)^2) / 2 + 4 EPS32, and 32 EPS32 (|y - beta| + |beta|) for the affine formula;
  * erf-GELU is 1.13-Lipschitz; its f32 evaluation adds 8 EPS32 |h|;
  * the 18-block tower: against the oracle with its 16-bit storage points (storage=), within the committed end-to-end tolerance
    of tests/test_convnext.py (fp16 4e-3, bf16 3e-2 of the features'
    spread); the per-stage bars above are what this module derives;
  * bit-exact: layout kernels == torch's .to(dtype) (round to nearest even, NaN compared as NaN), and every element a kernel
    must not write keeps its sentinel.
The fp16 and the bf16 library are both run.  Measured worst errors go through conftest.parity_log, as fractions of the bar.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import parity_log
from oracle import convnext_oracle as co

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64, I32, I64, U8 = (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64,
                                     torch.uint8)
DTYPES = pytest.mark.parametrize("T16", [F16, BF16], ids=["fp16", "bf16"])
MANT = {F16: 10, BF16: 7}
EMIN = {F16: -14, BF16: -126}
EPS32 = 2.0 ** -24
TOL_SUM = 1e-5
TRANS = 8 * EPS32
FORM = 32 * EPS32
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_num_threads(16)
    import multimodal_propaganda_meme_classification_amd as m
    from multimodal_propaganda_meme_classification_amd import ops as _ops
    m.ops = _ops
    yield m
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _name(T16):
    return "fp16" if T16 == F16 else "bf16"


def _lib(pkg, T16=BF16):
    return pkg._lib.load(_name(T16))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr()


def _ulp(ref, T16):
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** EMIN[T16]))
    return torch.pow(2.0, (e - 1 - MANT[T16]).to(F64))


def _r16(x64, T16):
    return x64.to(T16).to(F64)


def _same(got, exp):
    """bit-exact equality with NaN == NaN (payloads may differ)"""
    g, e = got.cpu(), exp.cpu()
    gn, en = torch.isnan(g.float()), torch.isnan(e.float())
    if not torch.equal(gn, en):
        return False
    ib = {2: torch.int16, 4: I32}[g.element_size()]
    return torch.equal(torch.where(gn, torch.zeros_like(g), g).view(ib), torch.where(en, torch.zeros_like(e), e).view(ib))


def _worst(got, ref, bar, what):
    err = (got - ref).abs()
    r = float((err / bar).max())
    assert torch.isfinite(got).all() and r <= 1.0, f"{what}: worst err/bar {r:.3f} (max err {float(err.max()):.3e})"
    return r


# ---- mh_dwconv_nhwc ------------------------------------------------------------------------------------------------------------

HWS = [(1, 1), (7, 7), (8, 8), (9, 13), (14, 21), (28, 28), (56, 56), (1, 64)]


def _tile(H, W):
    return 7 if (H % 8 and W % 8 and H % 7 == 0 and W % 7 == 0) else 8


@DTYPES
@pytest.mark.parametrize("Cc", [8, 96, 192, 200, 384, 768])
def test_dwconv_float64(pkg, T16, Cc):
    lib = _lib(pkg, T16)
    worst = 0.0
    tiles = set()
    for H, W in HWS:
        B = 1 if H * W * Cc > 500_000 else 2
        g = torch.Generator().manual_seed(H * 100 + W + Cc)
        x16 = torch.randn(B, Cc, H, W, generator=g).to(T16)
        w = torch.randn(Cc, 1, 7, 7, generator=g) / 7.0
        b = torch.randn(Cc, generator=g)
        x64 = x16.to(F64)
        conv = F.conv2d(x64, w.to(F64), None, padding=3, groups=Cc)
        sabs = F.conv2d(x64.abs(), w.to(F64).abs(), None, padding=3, groups=Cc)
        xd = x16.permute(0, 2, 3, 1).contiguous().cuda()
        wt = torch.empty((49, Cc), dtype=F32, device=DEV)
        wd = w.cuda()
        assert lib.mh_dwconv_weight_pack(_p(wd), _p(wt), Cc, 7, _st()) == 0
        assert torch.equal(wt.cpu(), w.reshape(Cc, 49).t())          # tap-major weight image
        tiles.add(_tile(H, W))
        for bias in (None, b):
            y = torch.full((B * H * W * Cc + 64,), NAN, dtype=T16, device=DEV)
            bd = None if bias is None else bias.cuda()
            assert lib.mh_dwconv_nhwc(_p(xd), _p(wt), None if bd is None else _p(bd), _p(y), B, H, W, Cc, 7, _st()) == 0
            ref = conv + (0 if bias is None else bias.to(F64)[None, :, None, None])
            bar = _ulp(ref, T16) + TOL_SUM * (sabs + (0 if bias is None else bias.to(F64).abs()[None, :, None, None]))
            got = y[:B * H * W * Cc].view(B, H, W, Cc).permute(0, 3, 1, 2).cpu().to(F64)
            worst = max(worst, _worst(got, ref, bar, f"dwconv {H}x{W} C{Cc} bias={bias is not None}"))
            assert torch.isnan(y[B * H * W * Cc:].float()).all().item()
    assert tiles == {7, 8}
    parity_log(f"[cnx dwconv C{Cc} {_name(T16)}] y {worst:.3e}")


# ---- the ConvNeXt launch plan: stem, one CNBlock, a downsampling layer ---------------------------------------------------------

def _model(pkg, T16, depths, dims, seed=3):
    p = co.init_params(seed=seed, depths=depths, dims=dims, num_classes=10)
    m = pkg.ConvNeXtTiny(num_classes=10, compute_dtype=_name(T16), depths=depths, dims=dims)
    m.load_state_dict(p, strict=True)
    return m.cuda().eval(), p


def _round_err(u, E, T16):
    """the kernel's unrounded value lies in [u - E, u + E]; rounding is monotone, so its 16-bit value differs from the reference's
    round(u) by at most this much (0 wherever no rounding midpoint lies inside the interval)"""
    r = _r16(u, T16)
    return torch.maximum((_r16(u + E, T16) - r).abs(), (_r16(u - E, T16) - r).abs())


def _ln_ref(t, e_in, gamma, beta, eps=1e-6):
    """LayerNorm over the last dim of t (f64, the 16-bit values the reference feeds forward), input bound e_in -> (y_u, f32 bound)"""
    D = t.shape[-1]
    mean = t.mean(-1, keepdim=True)
    c = t - mean
    var = (c * c).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    yhat = c * rstd
    g, b = gamma.to(F64), beta.to(F64)
    y = yhat * g + b
    prop = g.abs() * rstd * (e_in + e_in.mean(-1, keepdim=True) + yhat.abs() * (yhat.abs() * e_in).mean(-1, keepdim=True))
    dm = TOL_SUM * t.abs().sum(-1, keepdim=True) / D
    dr = (TOL_SUM + (dm / var.sqrt()) ** 2) / 2 + 4 * EPS32
    own = g.abs() * rstd * (dm + c.abs() * dr) + FORM * ((y - b).abs() + b.abs())
    return y, prop + own


def _linear_ref(a, e_a, w, b, residual=None):
    """z = a w^T + b (+ residual), a / w / b as the kernel reads them -> (z_u, f32 bound)"""
    w64 = w.to(F64)
    z = a @ w64.t() + b.to(F64)
    terms = a.abs() @ w64.abs().t() + b.to(F64).abs()
    if residual is not None:
        z = z + residual
        terms = terms + residual.abs()
    return z, e_a @ w64.abs().t() + TOL_SUM * terms


def _stem_ref(p, img, T16):
    """-> (y_u, f32 bound) of the stem's LayerNorm output"""
    B, _, H, W = img.shape
    c0 = p["features.0.0.weight"].shape[0]
    patches = img.to(T16).to(F64).view(B, 3, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(-1, 48)
    w0 = p["features.0.0.weight"].reshape(c0, 48).to(T16)
    z, E = _linear_ref(patches, torch.zeros_like(patches), w0, p["features.0.0.bias"])
    return _ln_ref(_r16(z, T16), _round_err(z, E, T16), p["features.0.1.weight"], p["features.0.1.bias"])


def _block_ref(p, q, x, B, h, w, d, T16):
    """one CNBlock from x (the kernel's block input, exact, f64 [B*h*w][d]) -> (out_u, f32 bound)"""
    x4 = x.view(B, h, w, d).permute(0, 3, 1, 2)
    wdw, bdw = p[q + "block.0.weight"].to(F64), p[q + "block.0.bias"].to(F64)
    t = F.conv2d(x4, wdw, bdw, padding=3, groups=d)
    Et = TOL_SUM * (F.conv2d(x4.abs(), wdw.abs(), None, padding=3, groups=d) + bdw.abs()[None, :, None, None])
    t, Et = t.permute(0, 2, 3, 1).reshape(-1, d), Et.permute(0, 2, 3, 1).reshape(-1, d)
    n, En = _ln_ref(_r16(t, T16), _round_err(t, Et, T16), p[q + "block.2.weight"], p[q + "block.2.bias"])
    z, Ez = _linear_ref(_r16(n, T16), _round_err(n, En, T16), p[q + "block.3.weight"].to(T16), p[q + "block.3.bias"])
    hid = F.gelu(z)
    Eh = 1.13 * Ez + TRANS * hid.abs()
    gamma = p[q + "layer_scale"].reshape(d)
    w2 = (gamma[:, None] * p[q + "block.5.weight"]).to(T16)          # folded as ConvNeXtTiny._packed folds it
    b2 = gamma * p[q + "block.5.bias"]
    return _linear_ref(_r16(hid, T16), _round_err(hid, Eh, T16), w2, b2, residual=x)


STAGES = [(96, (56, 56), (9, 13)), (192, (28, 28), (5, 11)), (384, (14, 14), (3, 7)), (768, (7, 7), (2, 5))]


@DTYPES
@pytest.mark.parametrize("d,full,ragged", STAGES, ids=[f"d{s[0]}" for s in STAGES])
def test_stem_and_cnblock(pkg, T16, d, full, ragged):
    worst_s = worst_b = 0.0
    m0, p = _model(pkg, T16, (0,), (d,))
    m1, p1 = _model(pkg, T16, (1,), (d,))
    for k in ("features.0.0.weight", "features.0.0.bias", "features.0.1.weight", "features.0.1.bias"):
        assert torch.equal(p[k], p1[k])         # the same stem: m0's output is m1's block input
    for h, w in (full, ragged):
        B = 2 if h * w < 1000 else 1
        img = torch.randn(B, 3, 4 * h, 4 * w, generator=torch.Generator().manual_seed(h * w + d))
        x0, *_ = m0._feature_map(img.cuda())
        x0 = x0.cpu().to(F64)
        s_ref, s_bar = _stem_ref(p, img, T16)
        worst_s = max(worst_s, _worst(x0, s_ref, s_bar + _ulp(s_ref, T16), f"stem d{d} {h}x{w}"))
        x1, *_ = m1._feature_map(img.cuda())
        o_ref, o_bar = _block_ref(p1, "features.1.0.", x0, B, h, w, d, T16)
        worst_b = max(worst_b, _worst(x1.cpu().to(F64), o_ref, o_bar + _ulp(o_ref, T16), f"cnblock d{d} {h}x{w}"))
    parity_log(f"[cnx stem d{d} {_name(T16)}] y {worst_s:.3e}")
    parity_log(f"[cnx cnblock d{d} {_name(T16)}] out {worst_b:.3e}")


@DTYPES
@pytest.mark.parametrize("d", [96, 192, 384])
def test_downsample(pkg, T16, d):
    m0, p = _model(pkg, T16, (0,), (d,))
    m2, p2 = _model(pkg, T16, (0, 0), (d, 2 * d))
    for k in ("features.0.0.weight", "features.0.0.bias", "features.0.1.weight", "features.0.1.bias"):
        assert torch.equal(p[k], p2[k])
    worst = 0.0
    for h, w in ((8, 8), (6, 10)):
        img = torch.randn(2, 3, 4 * h, 4 * w, generator=torch.Generator().manual_seed(d + h))
        x0, *_ = m0._feature_map(img.cuda())
        x0 = x0.cpu().to(F64)
        y, *_ = m2._feature_map(img.cuda())
        n, En = _ln_ref(x0, torch.zeros_like(x0), p2["features.2.0.weight"], p2["features.2.0.bias"])
        nr, en = _r16(n, T16), _round_err(n, En, T16)
        col = nr.view(2, h // 2, 2, w // 2, 2, d).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4 * d)       # (kh, kw, c) columns
        ecol = en.view(2, h // 2, 2, w // 2, 2, d).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4 * d)
        wk = p2["features.2.1.weight"].permute(0, 2, 3, 1).reshape(2 * d, 4 * d).to(T16)
        z, ez = _linear_ref(col, ecol, wk, p2["features.2.1.bias"])
        worst = max(worst, _worst(y.cpu().to(F64), z, ez + _ulp(z, T16), f"downsample d{d} {h}x{w}"))
    parity_log(f"[cnx downsample d{d} {_name(T16)}] out {worst:.3e}")


# ---- the whole tower -----------------------------------------------------------------------------------------------------------

TOWER_TOL = {F16: 4e-3, BF16: 3e-2}     # tests/test_convnext.py's committed end-to-end tolerance (relative to the features' spread),
#                                         here against the oracle with the tower's 16-bit storage points (storage=)


@DTYPES
@pytest.mark.parametrize("HW", [(32, 32), (64, 96), (96, 64), (224, 320)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tower_against_oracle(pkg, T16, HW):
    p = co.init_params(seed=5)
    m = pkg.ConvNeXtTiny(compute_dtype=_name(T16))
    m.load_state_dict(p, strict=True)
    m = m.cuda().eval()
    for B in (1, 3):
        x = torch.randn(B, 3, *HW, generator=torch.Generator().manual_seed(B + HW[1]))
        ref = co.convnext_pooled_features(p, x, storage=T16)
        got = m.pooled_features(x.cuda()).cpu()
        assert got.shape == (B, 768)
        spread = float(ref.std()) if ref.numel() > 1 else 1.0
        err = float((got - ref).abs().max()) / spread
        assert err < TOWER_TOL[T16], f"{HW} B={B}: {err}"
        parity_log(f"[cnx tower {HW[0]}x{HW[1]} B{B} {_name(T16)}] pooled {err / TOWER_TOL[T16]:.3e}")
        if B == 3:                                    # the classifier, from the kernel's own pooled features (read back)
            logits = m(x.cuda()).cpu().to(F64)
            pooled = _r16(got.to(F64), T16)
            n, En = _ln_ref(pooled, torch.zeros_like(pooled), p["classifier.0.weight"], p["classifier.0.bias"])
            z, Ez = _linear_ref(_r16(n, T16), _round_err(n, En, T16), p["classifier.2.weight"], p["classifier.2.bias"])
            assert logits.shape == (3, 1000)
            cls = _worst(logits, z, Ez, f"classifier {HW}")
    parity_log(f"[cnx classifier {HW[0]}x{HW[1]} {_name(T16)}] logits {cls:.3e}")


@DTYPES
def test_batch_independence_under_nonfinite_input(pkg, T16):
    """an Inf or NaN in the first pixel of image b+1 (the row right after image b's last one) must not reach image b"""
    p = co.init_params(seed=5)
    m = pkg.ConvNeXtTiny(compute_dtype=_name(T16))
    m.load_state_dict(p, strict=True)
    m = m.cuda().eval()
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    clean = m.pooled_features(x.cuda()).cpu()
    assert torch.isfinite(clean).all()
    for bad, val in ((1, NAN), (2, float("inf")), (0, -float("inf"))):
        y = x.clone()
        y[bad, :, 0, 0] = val
        got = m.pooled_features(y.cuda()).cpu()
        for i in range(3):
            if i != bad:
                assert torch.isfinite(got[i]).all() and torch.equal(got[i], clean[i]), f"image {bad} = {val} leaked into image {i}"
    parity_log(f"[cnx batch_independence {_name(T16)}] other images bit-identical to the clean run (NaN / +inf / -inf)")


# ---- layout kernels, bit-exact -------------------------------------------------------------------------------------------------

def _rne_ties(T16, n, g):
    """f32 values exactly halfway between two neighbouring 16-bit values (both parities), plus NaN / +-Inf"""
    base = torch.randn(n, generator=g).to(T16)
    nxt = (base.view(torch.int16) + 1).view(T16)                 # the neighbour one ulp further from zero
    return ((base.to(F64) + nxt.to(F64)) / 2).to(F32)            # exact in f32


@DTYPES
@pytest.mark.parametrize("Cp", [3, 4, 8])
def test_nchw_to_nhwc(pkg, T16, Cp):
    lib = _lib(pkg, T16)
    B, Cc, H, W = 2, 3, 5, 7
    g = torch.Generator().manual_seed(Cp)
    x = _rne_ties(T16, B * Cc * H * W, g).view(B, Cc, H, W)
    x[0, 0, 0, 0], x[1, 2, 4, 6], x[0, 1, 2, 3] = NAN, float("inf"), -float("inf")
    assert (x.to(F64) != x.to(T16).to(F64)).sum() > 50            # real ties
    y = torch.full((B * H * W * Cp + 8,), NAN, dtype=T16, device=DEV)
    xd = x.cuda()
    assert lib.mh_nchw_to_nhwc(_p(xd), _p(y), B, Cc, H, W, Cp, _st()) == 0
    exp = torch.zeros(B, H, W, Cp, dtype=T16)
    exp[..., :Cc] = x.permute(0, 2, 3, 1).to(T16)
    assert _same(y[:B * H * W * Cp].view(B, H, W, Cp), exp)
    assert torch.isnan(y[B * H * W * Cp:].float()).all().item()
    assert lib.mh_nchw_to_nhwc(_p(xd), _p(y), B, Cc, H, W, 2, _st()) != 0       # Cp < C
    parity_log(f"[cnx layout nchw_to_nhwc Cp{Cp} {_name(T16)}] == torch .to() (RNE ties, NaN, Inf), pad channels zero")


def _pack_ref(w, Cp, ldk, T16):
    Cout, Cin, KH, KW = w.shape
    t = torch.zeros(Cout, KH, KW, Cp)
    t[..., :Cin] = w.permute(0, 2, 3, 1)
    out = torch.zeros(Cout, ldk)
    out[:, :KH * KW * Cp] = t.reshape(Cout, -1)
    return out.to(T16)


PACKS = [(16, 8, 1, 1, 8, 8), (8, 3, 7, 7, 8, 7 * 7 * 8 + 16), (12, 5, 3, 3, 8, 80), (4, 16, 2, 2, 16, 72), (6, 64, 3, 3, 64, 576),
         (5, 7, 3, 2, 7, 48)]


@DTYPES
def test_conv_weight_pack_unpack(pkg, T16):
    lib = _lib(pkg, T16)
    for Cout, Cin, KH, KW, Cp, ldk in PACKS:
        g = torch.Generator().manual_seed(Cout * Cin + KH)
        w = torch.randn(Cout, Cin, KH, KW, generator=g)
        out = torch.full((Cout * ldk + 8,), NAN, dtype=T16, device=DEV)
        wd = w.cuda()
        assert lib.mh_conv_weight_pack(_p(wd), _p(out), Cout, Cin, KH, KW, Cp, ldk, _st()) == 0
        assert _same(out[:Cout * ldk].view(Cout, ldk), _pack_ref(w, Cp, ldk, T16)), (Cout, Cin, KH, KW, Cp, ldk)
        assert torch.isnan(out[Cout * ldk:].float()).all().item()
        gk = torch.randn(Cout, ldk, generator=g)
        gkd = gk.cuda()
        for scale in (1.0, 0.37, -3.0):
            gw = torch.full((Cout * Cin * KH * KW + 8,), NAN, device=DEV)
            assert lib.mh_conv_weight_unpack(_p(gkd), _p(gw), Cout, Cin, KH, KW, Cp, ldk, C.c_float(scale), _st()) == 0
            src = gk[:, :KH * KW * Cp].view(Cout, KH, KW, Cp)[..., :Cin].permute(0, 3, 1, 2)
            exp = torch.tensor(scale, dtype=F32) * src
            assert torch.equal(gw[:Cout * Cin * KH * KW].view(Cout, Cin, KH, KW).cpu(), exp), (Cout, Cin, KH, KW, scale)
            assert torch.isnan(gw[Cout * Cin * KH * KW:]).all().item()
    assert lib.mh_conv_weight_pack(_p(wd), _p(out), 4, 8, 3, 3, 8, 71, _st()) != 0       # ldk < KH KW Cp
    parity_log(f"[cnx layout conv_weight_pack/unpack {_name(T16)}] == torch permute + .to(), {len(PACKS)} shapes, 3 scales")


@DTYPES
def test_conv_weight_pack_batched_resnet50(pkg, T16):
    from multimodal_propaganda_meme_classification_amd import resnet
    lib = _lib(pkg, T16)
    net = resnet.ResNet50(compute_dtype=_name(T16))
    convs = [resnet._Conv(mod, cp) for mod, cp in net._convs()]
    assert len(convs) == 53
    ws = [c.mod.weight.detach().to(F32).contiguous().cuda() for c in convs]
    outs = [torch.full((c.cout, c.ldk), NAN, dtype=T16, device=DEV) for c in convs]
    jobs = (pkg._lib.MhConvPackJob * len(convs))()
    for j, (c, w, o) in enumerate(zip(convs, ws, outs)):
        jobs[j].w, jobs[j].out = _p(w), _p(o)
        jobs[j].Cout, jobs[j].Cin, jobs[j].KH, jobs[j].KW, jobs[j].Cp, jobs[j].ldk = c.cout, c.cin, c.kh, c.kw, c.cp, c.ldk
    assert lib.mh_conv_weight_pack_batched(jobs, len(convs), _st()) == 0
    for c, w, o in zip(convs, ws, outs):
        single = torch.full((c.cout, c.ldk), NAN, dtype=T16, device=DEV)
        assert lib.mh_conv_weight_pack(_p(w), _p(single), c.cout, c.cin, c.kh, c.kw, c.cp, c.ldk, _st()) == 0
        assert _same(o, single) and _same(o, _pack_ref(w.cpu(), c.cp, c.ldk, T16)), (c.cout, c.cin, c.kh, c.kw)
    big = (pkg._lib.MhConvPackJob * 65)()
    for j in range(65):
        big[j] = jobs[j % 53]
    assert lib.mh_conv_weight_pack_batched(big, 65, _st()) != 0
    parity_log(f"[cnx layout conv_weight_pack_batched {_name(T16)}] 53 ResNet-50 convolutions == single packs == reference")


def _patches_ref(img, P, T16):
    B, Cc, H, W = img.shape
    return img.view(B, Cc, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(-1, Cc * P * P).to(T16)


@DTYPES
@pytest.mark.parametrize("P", [8, 16, 32])
def test_patchify(pkg, T16, P):
    for Cc, H, W in ((2, 2 * P, 3 * P), (5, 3 * P, P)):
        g = torch.Generator().manual_seed(P + Cc)
        img = _rne_ties(T16, Cc * H * W * 2, g).view(2, Cc, H, W)
        img[1, Cc - 1, H - 1, W - 1] = NAN
        rows, K = 2 * (H // P) * (W // P), Cc * P * P
        out = torch.full((rows + 1, K), NAN, dtype=T16, device=DEV)
        pkg.ops.patchify(img.cuda(), P, out=out[:rows], dtype=T16)
        assert _same(out[:rows], _patches_ref(img, P, T16))
        assert torch.isnan(out[rows].float()).all().item()
    parity_log(f"[cnx layout patchify P{P} {_name(T16)}] == torch unfold + .to() (RNE ties), C 2 / 5, non-square")


@DTYPES
@pytest.mark.parametrize("P", [1, 4, 14, 16])
def test_patchify_ld(pkg, T16, P):
    for Cc, H, W in ((3, 2 * P, 3 * P), (2, 5 * P, 2 * P)):
        K = Cc * P * P
        ld = (K + 63) // 64 * 64 + (8 if K % 64 == 0 else 0)
        g = torch.Generator().manual_seed(P * 7 + Cc)
        img = _rne_ties(T16, Cc * H * W * 2, g).view(2, Cc, H, W)
        rows = 2 * (H // P) * (W // P)
        out = torch.full((rows + 1, ld), NAN, dtype=T16, device=DEV)
        pkg.ops.patchify(img.cuda(), P, out=out[:rows], dtype=T16, ld=ld)
        exp = torch.zeros(rows, ld, dtype=T16)
        exp[:, :K] = _patches_ref(img, P, T16)
        assert _same(out[:rows], exp), (P, Cc, H, W)
        assert torch.isnan(out[rows].float()).all().item()
    parity_log(f"[cnx layout patchify_ld P{P} {_name(T16)}] == torch unfold + .to(), pad columns zero over NaN")


def test_copy2d_u32(pkg):
    lib = pkg._lib.load()
    rows, cols, pad_to, ld_src, ld_dst = 7, 5, 9, 6, 13
    for dt in (BF16, F16, F32):
        wpe = 4 // torch.tensor([], dtype=dt).element_size()
        g = torch.Generator().manual_seed(wpe)
        src = torch.randn(rows * ld_dst * wpe, generator=g).to(dt).cuda()       # room for a wrong (larger) source pitch
        dst = torch.full((rows * ld_dst * wpe,), NAN, dtype=dt, device=DEV)
        pkg.ops.copy2d_words(src, ld_src, dst, ld_dst, rows, cols, pad_to)
        s = src.cpu().view(-1)[:rows * ld_src * wpe].view(rows, ld_src * wpe)
        d = dst.cpu().view(rows, ld_dst * wpe)
        assert _same(d[:, :cols * wpe], s[:, :cols * wpe])
        assert (d[:, cols * wpe:pad_to * wpe] == 0).all()
        assert torch.isnan(d[:, pad_to * wpe:].float()).all()            # words past pad_to untouched
        assert lib.mh_copy2d_u32(_p(src) + 2, ld_src, _p(dst), ld_dst, rows, cols, pad_to, _st()) != 0     # misaligned
        assert lib.mh_copy2d_u32(_p(src), ld_src, _p(dst) + 2, ld_dst, rows, cols, pad_to, _st()) != 0
        assert lib.mh_copy2d_u32(_p(src), ld_src, _p(dst), pad_to - 1, rows, cols, pad_to, _st()) != 0     # ld_dst < pad_to
    parity_log("[cnx layout copy2d_u32] 16-bit pairs and f32 copied bit for bit, pad zero, words past pad_to untouched")


def test_zero_rows(pkg):
    V, D = 40, 12
    table = torch.randn(V, D, generator=torch.Generator().manual_seed(1))
    ids = torch.tensor([3, 3, 0, V - 1, -1, V, V + 5, 17, 3, -100])
    t = table.cuda()
    pkg.ops.zero_rows(ids.cuda(), t)
    exp = table.clone()
    exp[[3, 0, V - 1, 17]] = 0
    assert torch.equal(t.cpu(), exp)
    parity_log("[cnx layout zero_rows] duplicate ids zeroed once, out-of-range ids ignored, other rows untouched")


@pytest.mark.parametrize("W", [4, 8, 228])
def test_image_normalize(pkg, W):
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for B, H in ((1, 1), (8, 3), (3, 1)):
        u8 = torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(W + B), dtype=U8)
        u8[0, 0, 0] = torch.tensor([0, 255, 128], dtype=U8)
        out = pkg.ops.image_normalize_u8(u8.cuda(), mean, std).cpu()
        x = u8.permute(0, 3, 1, 2).float() / 255
        exp = (x - torch.tensor(mean, dtype=F32)[None, :, None, None]) / torch.tensor(std, dtype=F32)[None, :, None, None]
        assert torch.equal(out, exp), (B, H, W)
    parity_log(f"[cnx layout image_normalize W{W}] == torch float32 x / 255, (x - mean) / std bit for bit")
