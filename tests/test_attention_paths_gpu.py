"""Every attention kernel path against one plain reference: float64 torch on the CPU, computed from the same 16-bit inputs.

Reference: scores q.k^T / 8, additive key mask (1 - mask) * finfo(float32).min as HF BERT applies it, softmax, dropout as P
times the kernels' own mask ops.dropout_mask(...) / (1 - p) at element ((b*H + h)*S + q_pos)*S + k_pos (the unpacked
positions, also for the packed form).  A row with no key to attend to (its sequence's key mask is all zeros) has, by the
convention of include/memehip.h, out = 0, lse = -inf and no gradient; the reference applies the same convention.

Which kernel each case reaches (csrc/attention.hip: launch_fwd, onepass_fits, launch_bwd, dual_pair, mh_attn_fwd_grouped,
mh_attn_bwd_grouped):

  S / mask / dropout                         forward                          backward
  ---------------------------------------------------------------------------------------------------------------------
  S <= 128 (1, 31, 32, 33, 64, 65, 127, 128) fwd <4, 2> (split 1 at S <= 128)  dq + dkv resident <4, 2>
  129..224 unmasked, dense, no dropout       fwd <7, 4>, one WG per head       one-pass (onepass 2, default);
     (129, 160, 197, 223, 224)                                                 7-wave streaming <7, 0> at onepass 0
  129..224 masked, packed or dropout         fwd <7, 4>                        7-wave streaming <7, 0>
  225..256 (225, 255, 256)                   fwd <4, 4>, split 2               4-wave streaming <4, 0>
  S > 256 (257, 300, 577)                    fwd <4, 0> streaming              4-wave streaming <4, 0>
  dropout p = 0.1 (33, 128, 160, 224, 256, 257, masked and not): the DROP = true twin of every row above

  grouped pair (one problem 129..224 without dropout + one <= 128; dual_pair):
    forward                       attn_fwd_dual_kernel<4, DROP_B>
    backward onepass 2            attn_bwd_onepass_dual_kernel<2, DROP_B>
    backward onepass 1            attn_bwd_onepass_kernel + attn_bwd_merged_single_kernel<2, DROP_B>
    backward onepass 0            attn_bwd_merged_dual_kernel<2, DROP_B>
  a pair with S_a = 240 is refused by dual_pair: separate launches of the rows above.

Packed masks hold empty sequences (first, middle, last), one-token sequences, lengths 31 / 32 / 33 / 64 / 65, holes, and
sequences of 200 and 300 rows; an empty mask row still keeps its pooled position as a query with no key (mh_pack_plan), and
a hand-built plan gives sequences of zero rows (Sb == 0).  Adversarial values (sharp, monotonically rising scores, a V with
a large common offset) push the lazy running maximum and the delta = rowsum(dO o O) cancellation.

Every row of the table is held to three things (tests/attention_restatement.py holds the case generator, the bound and its
derivation; tests/test_attention_bounds.py validates both without a GPU):

  old bars      those of tests/test_kernels_gpu.py::test_attention_fwd_bwd (out 1e-2 / 6e-3, lse 1e-3 / 2e-3, dqkv 2e-2 / 1.5e-2 *
                max |dqkv|), unchanged.  They let through a few percent of error on a subset of elements.
  derived bound out, lse, dQ, dK and dV each against their own per-element first-order bound, computed in float64 from the
                reference's intermediates (one term per rounding of the kernels, doubled once): every random and adversarial test
                below.  The worst error / bound per tensor goes through conftest.parity_log.
  exact case    tied scores (every query's best score shared by 1, 2 or 4 keys, every other key >= 128 below): out, dQ, dK, dV
                must equal the float64 reference bit for bit in fp16 and in bf16 (torch.equal), lse stays on the bound.  The
                test_exact_* twins of every row: the dense table plus S = 577 under the same onepass modes, dropout at p = 0.5
                (multiplier exactly 2), the packed masks and zero-length plans, every grouped pair in both orders under onepass
                2 / 1 / 0 with the S_a = 240 refusal, and two wide-head geometries (B = 2, H = 12, S = 197 and B = 1, H = 16,
                S = 577: the row pitches of BERT-base and ViT-L).  Rounding points that keep it exact, read in attn_fwd_body,
                attn_bwd_dq_body, attn_bwd_dkv_body and attn_bwd_onepass_body (the dual and merged kernels call these bodies):
                tied keys see identical arithmetic, so exp2(st - m) = 1 and the others exp2(<= -184) = 0; a lazy-maximum move
                rescales by alpha = 0 exactly; l and the PV sums are small integers, 1 / l a power of two; the backward's
                p = exp2(s c - lse log2(e)) is 1/n to ~2^-16, and p o M and p (dP - delta) are rounded to the 16-bit operand
                (acc_frag, the one-pass mailbox), whose true values are representable; delta is summed from an exact stored O.
                No path needed the 1-ulp fallback.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

import attention_restatement as R
from conftest import parity_log

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
TOL = dict(out=(1e-2, 6e-3), lse=(1e-3, 2e-3), dqkv=(2e-2, 1.5e-2))
P_DROP = 0.1
P_TIED = 0.5            # the exact case's dropout: mh_drop_ctx's scale 1.0f / (1.0f - p) is exactly 2


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_propaganda_meme_classification_amd import ops as _ops
    return _ops


def _rng_words(seed):
    return torch.tensor([seed & 0x7FFFFFFF, 0, 3, 0], dtype=torch.int32, device="cuda")


def _prefix_mask(B, S, lens):
    return torch.from_numpy(R.prefix_mask(S, lens)).cuda()


def _drop_probs(ops, B, H, S, drop):
    """the kernels' dropout multipliers of the probabilities, [B, H, S(query), S(key)] by unpacked position"""
    if drop is None:
        return None
    keep = ops.dropout_mask(B * H * S * S, drop, "cuda")
    assert bool((keep <= 1).all()), "dropout_mask returns something other than 0 and 1"
    return keep.to(F64).cpu().view(B, H, S, S) / (1.0 - drop[1])


@contextlib.contextmanager
def _onepass(ops, t, mode):
    lib = ops._L(t)
    lib.mh_attn_set_onepass(int(mode))
    try:
        yield
    finally:
        lib.mh_attn_set_onepass(2)


def _reference(qkv, mask, dout, B, S, H, pm=None, exact=False):
    """float64 out [B*S, H*64], lse [B, H, S], dqkv [B*S, 3*H*64] from the 16-bit inputs (dense positions), and the derived bound
    of each in the same layout (R.bounds); exact: the tied case, whose reference the kernels must reproduce bit for bit."""
    r = R.reference(qkv, dout, B, S, H, mask, pm, flush=exact)
    if exact:
        for n in ("O", "dQ", "dK", "dV"):
            assert R.representable(getattr(r, n).contiguous(), qkv.dtype), f"tied case: {n} is not exact in {qkv.dtype}"
        z = torch.zeros_like(r.O)
        bd = dict(R.bounds(r, qkv.dtype, lse_only=True), out=z, dQ=z, dK=z, dV=z)
    else:
        bd = R.bounds(r, qkv.dtype)
    return dict(out=R.rows(r.O), lse=r.lse, dqkv=R.rows3(r.dQ, r.dK, r.dV), b_out=R.rows(bd["out"]), b_lse=bd["lse"],
                b_dqkv=R.rows3(bd["dQ"], bd["dK"], bd["dV"]), exact=exact, dtype=qkv.dtype)


def _check(what, got, want, kind, scale=None):
    """elementwise |got - want| <= rtol |want| + atol (* scale); infinite references must be matched exactly.
    Returns the worst absolute error, for the parity log."""
    rtol, atol = TOL[kind]
    got = got.detach().cpu().to(F64)
    want = want.detach().cpu().to(F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = torch.isfinite(want)
    assert torch.equal(got[~fin], want[~fin]), f"{what}: rows with no key: expected {want[~fin][:4].tolist()}, got {got[~fin][:4].tolist()}"
    assert torch.isfinite(got[fin]).all(), f"{what}: {int((~torch.isfinite(got[fin])).sum())} non-finite values"
    g, w = got[fin], want[fin]
    s = 1.0 if scale is None else scale
    err = (g - w).abs()
    bad = err > atol * s + rtol * w.abs()
    worst = float(err.max()) if err.numel() else 0.0
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {worst:.4g} "
                           f"(atol {atol * s:.4g}, ref max {float(w.abs().max()):.4g})")
    return worst


def _check_all(tag, out, lse, dqkv, ref, H):
    """the exact case: out / dQ / dK / dV bit for bit, lse on its bound.  Every other case: the old bars (dQ, dK, dV reported
    separately, tolerance scaled by max |dqkv| as before), then each tensor against its own derived bound."""
    g = dqkv.detach().cpu().view(-1, 3, H * 64)
    w = ref["dqkv"].view(-1, 3, H * 64)
    bw = ref["b_dqkv"].view(-1, 3, H * 64)
    if ref["exact"]:
        dt = ref["dtype"]
        for n, got, want in [("out", out.detach().cpu(), ref["out"])] + [(f"d{n}", g[:, i], w[:, i]) for i, n in enumerate("QKV")]:
            if not torch.equal(got, want.to(dt)):
                diff = got.to(F64) != want
                raise AssertionError(f"{tag} {n}: {int(diff.sum())}/{diff.numel()} elements differ from the exact result, "
                                     f"max |diff| {float((got.to(F64) - want).abs().max()):.4g}")
        r_lse = R.ratio(lse, ref["lse"], ref["b_lse"])
        parity_log(f"[attention {tag}] out dQ dK dV bit-exact; lse error / bound {r_lse:.3f}")
        assert r_lse <= 1.0, f"{tag} lse: {r_lse:.3f} of the derived bound"
        return
    e_out = _check(f"{tag} out", out, ref["out"], "out")
    e_lse = _check(f"{tag} lse", lse, ref["lse"], "lse")
    scale = max(float(ref["dqkv"].abs().max()), 1e-30)
    e = [_check(f"{tag} d{n}", g[:, i], w[:, i], "dqkv", scale) for i, n in enumerate("QKV")]
    parity_log(f"[attention {tag}] max err out {e_out:.3e} lse {e_lse:.3e} dQ {e[0]:.3e} dK {e[1]:.3e} dV {e[2]:.3e} "
               f"(max |dqkv| {scale:.3e})")
    rt = dict(out=R.ratio(out, ref["out"], ref["b_out"]), lse=R.ratio(lse, ref["lse"], ref["b_lse"]))
    for i, n in enumerate("QKV"):
        rt[f"d{n}"] = R.ratio(g[:, i], w[:, i], bw[:, i])
    parity_log(f"[attention bound {tag}] worst error / bound " + " ".join(f"{n} {v:.3f}" for n, v in rt.items()))
    for n, v in rt.items():
        assert v <= 1.0, f"{tag} {n}: {v:.3f} of the derived bound"


def _inputs(data, B, S, H, dtype, seed, mask=None):
    """'random': N(0, 1) rounded to dtype; 'tied': the exact case over the keys `mask` keeps"""
    if data == "tied":
        m = None if mask is None else mask.detach().cpu().numpy()
        qkv, dout = R.tied_case(B, S, H, m, R.tied_seed(B, S, H))
        return qkv.to(dtype).cuda(), dout.to(dtype).cuda()
    return R.dense_inputs(B, S, H, dtype, seed, "cuda")


# ---------------------------------------------------------------------------------------------------------------------
# 1. dense dispatch table
# ---------------------------------------------------------------------------------------------------------------------

S_TABLE = R.S_TABLE
_lens = R.lens
NAME = {"random": "", "tied": "exact "}


def _dense_case(ops, B, S, H, dtype, masked, data, seed, p_drop=None, rng=None, site=21):
    mask = _prefix_mask(B, S, _lens(S)) if masked else None
    qkv, dout = _inputs(data, B, S, H, dtype, seed, mask)
    drop = (_rng_words(S if rng is None else rng), p_drop, site) if p_drop else None
    ref = _reference(qkv, mask, dout, B, S, H, _drop_probs(ops, B, H, S, drop), exact=data == "tied")
    out, lse = ops.attn_fwd(qkv, mask, B, S, H, drop=drop)
    modes = (2, 0) if (129 <= S <= 224 and not masked and not drop) else (2,)
    for mode in modes:
        with _onepass(ops, qkv, mode):
            dqkv = ops.attn_bwd(qkv, mask, out, dout, lse, B, S, H, drop=drop)
            torch.cuda.synchronize()
        tag = f"{NAME[data]}dense{' dropout' if drop else ''} B={B} H={H} S={S} {'masked' if masked else 'unmasked'} {dtype}"
        _check_all(tag + ("" if drop else f" onepass={mode}"), out, lse, dqkv, ref, H)


@DTYPES
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("S", S_TABLE)
def test_dense_dispatch_table(ops, S, masked, dtype):
    _dense_case(ops, 3, S, 2, dtype, masked, "random", seed=S)


@DTYPES
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("S", S_TABLE + [577])
def test_exact_dense(ops, S, masked, dtype):
    _dense_case(ops, 3, S, 2, dtype, masked, "tied", seed=None)


@DTYPES
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("S", R.S_DROPOUT)
def test_dense_dropout(ops, S, masked, dtype):
    _dense_case(ops, 3, S, 2, dtype, masked, "random", seed=S + 500, p_drop=P_DROP)


@DTYPES
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("S", R.S_DROPOUT)
def test_exact_dense_dropout(ops, S, masked, dtype):
    _dense_case(ops, 3, S, 2, dtype, masked, "tied", seed=None, p_drop=P_TIED)


@DTYPES
@pytest.mark.parametrize("B,H,S", [(2, 12, 197), (1, 16, 577)], ids=["bert-base-pitch", "vit-l-pitch"])
def test_exact_wide_heads(ops, B, H, S, dtype):
    """row pitches 3 * 768 and 3 * 1024 elements instead of the 384 / 576 of H = 2 / 3 everywhere else in this module"""
    _dense_case(ops, B, S, H, dtype, False, "tied", seed=None)


# ---------------------------------------------------------------------------------------------------------------------
# 2. packed form vs the dense reference on the original positions
# ---------------------------------------------------------------------------------------------------------------------

def _packed_mask(case):
    """[B, S] int64 masks; empty rows are all zeros (R.packed_mask: empty first / middle / last, one token, the 32 / 64
    boundaries, holes, sequences of 200 and 300 rows)"""
    return torch.from_numpy(R.packed_mask(case)).cuda()


def _check_packed(tag, ops, plan, out_p, lse_p, dqkv_p, ref, B, S, H):
    """live rows against the reference at their original positions; rows >= n_rows stay exactly zero"""
    n = int(plan["n_rows"])
    rm = plan["row_map"][:n].long().cpu()
    cu = plan["cu"].long().cpu()
    b = rm // S
    pos = rm % S
    local = torch.arange(n) - cu[b]
    lse_c = lse_p.detach().cpu().view(B, H, S)
    got_lse = lse_c[b, :, local]                              # [n, H]
    sub = dict(ref, out=ref["out"][rm], lse=ref["lse"][b, :, pos], dqkv=ref["dqkv"][rm], b_out=ref["b_out"][rm],
               b_lse=ref["b_lse"][b, :, pos], b_dqkv=ref["b_dqkv"][rm])
    _check_all(tag, out_p[:n], got_lse, dqkv_p[:n], sub, H)
    if n < out_p.shape[0]:
        assert float(out_p[n:].float().abs().max()) == 0.0, f"{tag}: out rows past n_rows written"
        assert float(dqkv_p[n:].float().abs().max()) == 0.0, f"{tag}: dqkv rows past n_rows written"


def _packed_case(ops, case, dropout, dtype, data):
    mask = _packed_mask(case)
    B, S = mask.shape
    H = 2
    plan = ops.pack_plan(mask, 0)
    qkv, dout = _inputs(data, B, S, H, dtype, B * S, mask)
    keep = (mask != 0).clone()
    keep[:, 0] = True                                        # the pooled position is always a row of the packed stream
    dout = dout * keep.reshape(-1, 1).to(dtype)              # nothing downstream reads the dropped rows
    drop = (_rng_words(B + S), P_TIED if data == "tied" else P_DROP, 33) if dropout else None
    ref = _reference(qkv, mask, dout, B, S, H, _drop_probs(ops, B, H, S, drop), exact=data == "tied")
    qkv_p, dout_p = ops.pack_rows(qkv, plan, 3 * H * 64), ops.pack_rows(dout, plan, H * 64)
    out_p, lse_p = ops.attn_fwd_packed(qkv_p, plan, B, S, H, drop=drop)
    dqkv_p = ops.attn_bwd_packed(qkv_p, plan, out_p, dout_p, lse_p, B, S, H, drop=drop)
    torch.cuda.synchronize()
    _check_packed(f"{NAME[data]}packed {case} {'drop' if dropout else 'nodrop'} {dtype}", ops, plan, out_p, lse_p, dqkv_p, ref,
                  B, S, H)


@DTYPES
@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("case", R.PACKED_CASES)
def test_packed_vs_reference(ops, case, dropout, dtype):
    _packed_case(ops, case, dropout, dtype, "random")


@DTYPES
@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("case", R.PACKED_CASES)
def test_exact_packed(ops, case, dropout, dtype):
    _packed_case(ops, case, dropout, dtype, "tied")


def _zero_length_case(ops, S, dropout, dtype, data):
    B, H = 5, 2
    lens = R.zero_length_lens(S)
    mask = _prefix_mask(B, S, lens)
    m = mask.cpu().numpy().reshape(-1)
    dense = np.flatnonzero(m)
    n = len(dense)
    cu = np.zeros(B + 1, np.int32)
    cu[1:] = np.cumsum(lens)
    row_map = np.full(B * S, -1, np.int32)
    row_map[:n] = dense
    plan = dict(cu=torch.from_numpy(cu).cuda(), row_map=torch.from_numpy(row_map).cuda(),
                pmask=torch.ones(n, dtype=torch.int64, device="cuda"), n_rows=torch.tensor([n], dtype=torch.int32))
    qkv, dout = _inputs(data, B, S, H, dtype, S + 77, mask)
    dout = dout * mask.reshape(-1, 1).to(dtype)
    drop = (_rng_words(S + 5), P_TIED if data == "tied" else P_DROP, 45) if dropout else None
    ref = _reference(qkv, mask, dout, B, S, H, _drop_probs(ops, B, H, S, drop), exact=data == "tied")
    idx = torch.from_numpy(dense).long().cuda()
    qkv_p = torch.zeros_like(qkv)
    qkv_p[:n] = qkv[idx]
    dout_p = torch.zeros_like(dout)
    dout_p[:n] = dout[idx]
    out_p, lse_p = ops.attn_fwd_packed(qkv_p, plan, B, S, H, drop=drop)
    dqkv_p = ops.attn_bwd_packed(qkv_p, plan, out_p, dout_p, lse_p, B, S, H, drop=drop)
    torch.cuda.synchronize()
    _check_packed(f"{NAME[data]}packed Sb=0 S={S} {'drop' if dropout else 'nodrop'} {dtype}", ops, plan, out_p, lse_p, dqkv_p,
                  ref, B, S, H)
    lse_c = lse_p.cpu().view(B, H, S)
    for b in (0, 2, 4):
        assert float(lse_c[b].abs().max()) == 0.0, f"lse of the empty sequence {b} written"


@DTYPES
@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("S", [40, 200, 300])
def test_packed_zero_length_sequences(ops, S, dropout, dtype):
    """A hand-built plan (no pooled row kept) with sequences of zero rows first, in the middle and last: those workgroups
    write nothing, read no key mask word, and the neighbours are exact.  The packed key mask holds exactly n_rows words."""
    _zero_length_case(ops, S, dropout, dtype, "random")


@DTYPES
@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("S", [40, 200, 300])
def test_exact_packed_zero_length_sequences(ops, S, dropout, dtype):
    _zero_length_case(ops, S, dropout, dtype, "tied")


# ---------------------------------------------------------------------------------------------------------------------
# 3. grouped pairs (dual kernels) vs the reference
# ---------------------------------------------------------------------------------------------------------------------

def _grouped_case(ops, Sa, St, text, dtype, data):
    Ba, Ha, Bt, Ht = 2, 3, 3, 2
    mask = torch.from_numpy(R.text_mask(St)).cuda()          # a hole: packed index != position from there on
    qa, da = _inputs(data, Ba, Sa, Ha, dtype, Sa)
    qt, dt = _inputs(data, Bt, St, Ht, dtype, 1000 + St, mask)
    if text != "masked":                                     # packed: the dropped (padding) rows carry no gradient
        keep = (mask != 0).clone()
        keep[:, 0] = True
        dt = dt * keep.reshape(-1, 1).to(dtype)
    drop = (_rng_words(St + Sa), P_TIED if data == "tied" else P_DROP, 17) if text == "packed_drop" else None
    ref_a = _reference(qa, None, da, Ba, Sa, Ha, exact=data == "tied")
    ref_t = _reference(qt, mask, dt, Bt, St, Ht, _drop_probs(ops, Bt, Ht, St, drop), exact=data == "tied")
    if text == "masked":
        extra = dict(key_mask=mask)
        qt_in, dt_in = qt, dt
    else:
        plan = ops.pack_plan(mask, 0)
        extra = dict(key_mask=plan["pmask"], cu=plan["cu"], row_map=plan["row_map"])
        qt_in = ops.pack_rows(qt, plan, 3 * Ht * 64)
        dt_in = ops.pack_rows(dt, plan, Ht * 64)
    z = torch.zeros_like
    pa = dict(qkv=qa, out=z(da), lse=torch.zeros((Ba, Ha, Sa), device="cuda"), dout=da,
              delta=torch.zeros((Ba, Ha, Sa), device="cuda"), dqkv=z(qa), B=Ba, S=Sa, H=Ha)
    pt = dict(qkv=qt_in, out=z(dt_in), lse=torch.zeros((Bt, Ht, St), device="cuda"), dout=dt_in,
              delta=torch.zeros((Bt, Ht, St), device="cuda"), dqkv=z(qt_in), B=Bt, S=St, H=Ht, drop=drop, **extra)
    for mode in (2, 1, 0):
        for order, oname in (([pa, pt], "AB"), ([pt, pa], "BA")):
            for d in order:
                for k in ("out", "lse", "delta", "dqkv"):
                    d[k].zero_()
            with _onepass(ops, qa, mode):
                ops.attn_grouped(order, backward=False)
                ops.attn_grouped(order, backward=True)
                torch.cuda.synchronize()
            tag = f"{NAME[data]}grouped Sa={Sa} St={St} {text} {dtype} onepass={mode} {oname}"
            _check_all(tag + " A", pa["out"], pa["lse"], pa["dqkv"], ref_a, Ha)
            if text == "masked":
                _check_all(tag + " B", pt["out"], pt["lse"], pt["dqkv"], ref_t, Ht)
            else:
                _check_packed(tag + " B", ops, plan, pt["out"], pt["lse"], pt["dqkv"], ref_t, Bt, St, Ht)


@DTYPES
@pytest.mark.parametrize("text", ["masked", "packed", "packed_drop"])
@pytest.mark.parametrize("St", [1, 77, 128])
@pytest.mark.parametrize("Sa", [129, 197, 224, 240])
def test_grouped_pair_vs_reference(ops, Sa, St, text, dtype):
    """ViT-like problem A (unmasked) + text problem B in one grouped call, both orders, under onepass 2 / 1 / 0.
    Sa = 240 is refused by dual_pair: the separate launches."""
    _grouped_case(ops, Sa, St, text, dtype, "random")


@DTYPES
@pytest.mark.parametrize("text", ["masked", "packed", "packed_drop"])
@pytest.mark.parametrize("St", [1, 77, 128])
@pytest.mark.parametrize("Sa", [129, 197, 224, 240])
def test_exact_grouped_pair(ops, Sa, St, text, dtype):
    _grouped_case(ops, Sa, St, text, dtype, "tied")


# ---------------------------------------------------------------------------------------------------------------------
# 4. adversarial values
# ---------------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("kind", ["sharp", "rising", "offset"])
@pytest.mark.parametrize("S", [64, 197, 577])
def test_adversarial_scores(ops, S, kind, dtype):
    """R.adversarial: sharp (|score| up to ~60), rising (the running maximum moves on every sub-tile), offset (delta from the
    stored O is a difference of large terms; the bound's delta term is the one that holds it)"""
    B, H = 2, 3
    qkv, dout = R.adversarial(kind, B, S, H, dtype, S * 7 + len(kind), "cuda")
    ref = _reference(qkv, None, dout, B, S, H)
    if kind == "sharp":
        assert float(ref["lse"].max()) > 30.0
    out, lse = ops.attn_fwd(qkv, None, B, S, H)
    dqkv = ops.attn_bwd(qkv, None, out, dout, lse, B, S, H)
    torch.cuda.synchronize()
    _check_all(f"adversarial {kind} S={S} {dtype}", out, lse, dqkv, ref, H)


# ---------------------------------------------------------------------------------------------------------------------
# 5. a dense row with no key to attend to
# ---------------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("S", [64, 197, 300])
def test_fully_masked_dense_row(ops, S, dropout, dtype):
    """Batch row 1's key mask is all zeros: its out and dqkv rows are exactly 0 and its lse is -inf (include/memehip.h);
    no NaN reaches the other rows or heads."""
    B, H = 3, 2
    qkv, dout = _inputs("random", B, S, H, dtype, S + 300)
    mask = _prefix_mask(B, S, [S, 0, max(1, S // 2)])
    drop = (_rng_words(S + 9), P_DROP, 9) if dropout else None
    ref = _reference(qkv, mask, dout, B, S, H, _drop_probs(ops, B, H, S, drop))
    out, lse = ops.attn_fwd(qkv, mask, B, S, H, drop=drop)
    dqkv = ops.attn_bwd(qkv, mask, out, dout, lse, B, S, H, drop=drop)
    torch.cuda.synchronize()
    rows = slice(S, 2 * S)
    assert float(out[rows].float().abs().max()) == 0.0
    assert float(dqkv[rows].float().abs().max()) == 0.0
    assert bool((lse[1] == -math.inf).all())
    _check_all(f"fully masked row S={S} {'drop' if dropout else 'nodrop'} {dtype}", out, lse, dqkv, ref, H)
