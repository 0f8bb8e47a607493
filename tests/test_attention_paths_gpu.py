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

Tolerances are today's of tests/test_kernels_gpu.py::test_attention_fwd_bwd (out 1e-2 / 6e-3, lse 1e-3 / 2e-3, dqkv
2e-2 / 1.5e-2 * max |dqkv|); measured errors go through conftest.parity_log.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

from conftest import parity_log

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
TOL = dict(out=(1e-2, 6e-3), lse=(1e-3, 2e-3), dqkv=(2e-2, 1.5e-2))
P_DROP = 0.1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_propaganda_meme_classification_amd import ops as _ops
    return _ops


def _randn(shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda") * scale


def _rng_words(seed):
    return torch.tensor([seed & 0x7FFFFFFF, 0, 3, 0], dtype=torch.int32, device="cuda")


def _prefix_mask(B, S, lens):
    return (torch.arange(S)[None] < torch.tensor(lens)[:, None]).to(torch.int64).cuda()


def _drop_probs(ops, B, H, S, drop):
    """the kernels' dropout multipliers of the probabilities, [B, H, S(query), S(key)] by unpacked position"""
    if drop is None:
        return None
    return ops.dropout_mask(B * H * S * S, drop, "cuda").to(F64).cpu().view(B, H, S, S) / (1.0 - drop[1])


@contextlib.contextmanager
def _onepass(ops, t, mode):
    lib = ops._L(t)
    lib.mh_attn_set_onepass(int(mode))
    try:
        yield
    finally:
        lib.mh_attn_set_onepass(2)


def _reference(qkv, mask, dout, B, S, H, pm=None):
    """float64 out [B*S, H*64], lse [B, H, S], dqkv [B*S, 3*H*64] from the 16-bit inputs (dense positions)."""
    x = qkv.detach().cpu().to(F64).requires_grad_(True)
    q, k, v = x.view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    sc = q @ k.transpose(-1, -2) / 8.0
    dead = torch.zeros(B, dtype=torch.bool)
    if mask is not None:
        m = mask.detach().cpu().to(F64).view(B, S)
        sc = sc + (1.0 - m)[:, None, None, :] * torch.finfo(torch.float32).min
        dead = m.sum(1) == 0
    p = torch.softmax(sc, -1)
    lse = torch.logsumexp(sc, -1)
    if pm is not None:
        p = p * pm
    o = (p @ v).permute(0, 2, 1, 3).reshape(B * S, H * 64)
    d = dout.detach().cpu().to(F64)
    rows = dead.repeat_interleave(S)[:, None]
    o = o.masked_fill(rows, 0.0)                          # no key to attend to: out = 0, lse = -inf, no gradient
    lse = lse.masked_fill(dead[:, None, None], -math.inf)
    o.backward(d.masked_fill(rows, 0.0))
    return o.detach(), lse.detach(), x.grad


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
    """out / lse / dqkv against the reference; dQ, dK, dV reported separately, tolerance scaled by max |dqkv| as today"""
    r_out, r_lse, r_dqkv = ref
    e_out = _check(f"{tag} out", out, r_out, "out")
    e_lse = _check(f"{tag} lse", lse, r_lse, "lse")
    scale = max(float(r_dqkv.abs().max()), 1e-30)
    g = dqkv.detach().cpu().to(F64).view(-1, 3, H * 64)
    w = r_dqkv.view(-1, 3, H * 64)
    e = [_check(f"{tag} d{n}", g[:, i], w[:, i], "dqkv", scale) for i, n in enumerate("QKV")]
    parity_log(f"[attention {tag}] max err out {e_out:.3e} lse {e_lse:.3e} dQ {e[0]:.3e} dK {e[1]:.3e} dV {e[2]:.3e} "
               f"(max |dqkv| {scale:.3e})")


def _dense_inputs(B, S, H, dtype, seed):
    qkv = _randn((B * S, 3 * H * 64), seed).to(dtype)
    dout = _randn((B * S, H * 64), seed + 1).to(dtype)
    return qkv, dout


# ---------------------------------------------------------------------------------------------------------------------
# 1. dense dispatch table
# ---------------------------------------------------------------------------------------------------------------------

S_TABLE = [1, 31, 32, 33, 64, 65, 127, 128, 129, 160, 197, 223, 224, 225, 255, 256, 257, 300]


def _lens(S):
    return [S, max(1, S - 1), max(1, (S + 1) // 2)]          # full, last key masked, half


@DTYPES
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("S", S_TABLE)
def test_dense_dispatch_table(ops, S, masked, dtype):
    B, H = 3, 2
    qkv, dout = _dense_inputs(B, S, H, dtype, seed=S)
    mask = _prefix_mask(B, S, _lens(S)) if masked else None
    ref = _reference(qkv, mask, dout, B, S, H)
    out, lse = ops.attn_fwd(qkv, mask, B, S, H)
    modes = (2, 0) if (129 <= S <= 224 and not masked) else (2,)
    for mode in modes:
        with _onepass(ops, qkv, mode):
            dqkv = ops.attn_bwd(qkv, mask, out, dout, lse, B, S, H)
            torch.cuda.synchronize()
        _check_all(f"dense S={S} {'masked' if masked else 'unmasked'} {dtype} onepass={mode}", out, lse, dqkv, ref, H)


@DTYPES
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("S", [33, 128, 160, 224, 256, 257])
def test_dense_dropout(ops, S, masked, dtype):
    B, H = 3, 2
    qkv, dout = _dense_inputs(B, S, H, dtype, seed=S + 500)
    mask = _prefix_mask(B, S, _lens(S)) if masked else None
    drop = (_rng_words(S), P_DROP, 21)
    ref = _reference(qkv, mask, dout, B, S, H, _drop_probs(ops, B, H, S, drop))
    out, lse = ops.attn_fwd(qkv, mask, B, S, H, drop=drop)
    dqkv = ops.attn_bwd(qkv, mask, out, dout, lse, B, S, H, drop=drop)
    torch.cuda.synchronize()
    _check_all(f"dense dropout S={S} {'masked' if masked else 'unmasked'} {dtype}", out, lse, dqkv, ref, H)


# ---------------------------------------------------------------------------------------------------------------------
# 2. packed form vs the dense reference on the original positions
# ---------------------------------------------------------------------------------------------------------------------

def _packed_mask(case):
    """[B, S] int64 masks; empty rows are all zeros"""
    if case == "edges":                      # empty first / middle / last, one token, the 32 / 64 boundaries
        S, lens = 80, [0, 1, 31, 0, 32, 33, 64, 65, 0]
        m = np.arange(S)[None] < np.array(lens)[:, None]
    elif case == "holes":
        S = 96
        g = np.random.default_rng(7)
        m = g.random((5, S)) < 0.5
        m[0, 0] = m[2, 0] = True
        m[1, 0] = False                      # the pooled row (position 0) is kept as a query but is no key
        m[3] = False                         # empty
        m[4, 40:] = False
    elif case == "s200":
        S, lens = 200, [200, 0, 129, 161]
        m = np.arange(S)[None] < np.array(lens)[:, None]
    elif case == "s300":
        S = 300
        g = np.random.default_rng(9)
        m = np.arange(S)[None] < np.array([300, 1, 0, 257])[:, None]
        m[0] &= g.random(S) < 0.7
        m[0, 0] = True
    else:
        raise ValueError(case)
    return torch.from_numpy(m.astype(np.int64)).cuda()


def _check_packed(tag, ops, plan, out_p, lse_p, dqkv_p, ref, B, S, H):
    """live rows against the reference at their original positions; rows >= n_rows stay exactly zero"""
    n = int(plan["n_rows"])
    rm = plan["row_map"][:n].long().cpu()
    cu = plan["cu"].long().cpu()
    r_out, r_lse, r_dqkv = ref
    b = rm // S
    pos = rm % S
    local = torch.arange(n) - cu[b]
    lse_c = lse_p.detach().cpu().view(B, H, S)
    got_lse = lse_c[b, :, local]                              # [n, H]
    want_lse = r_lse[b, :, pos]
    _check_all(tag, out_p[:n], got_lse, dqkv_p[:n], (r_out[rm], want_lse, r_dqkv[rm]), H)
    if n < out_p.shape[0]:
        assert float(out_p[n:].float().abs().max()) == 0.0, f"{tag}: out rows past n_rows written"
        assert float(dqkv_p[n:].float().abs().max()) == 0.0, f"{tag}: dqkv rows past n_rows written"


@DTYPES
@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("case", ["edges", "holes", "s200", "s300"])
def test_packed_vs_reference(ops, case, dropout, dtype):
    mask = _packed_mask(case)
    B, S = mask.shape
    H = 2
    plan = ops.pack_plan(mask, 0)
    qkv, dout = _dense_inputs(B, S, H, dtype, seed=B * S)
    keep = (mask != 0).clone()
    keep[:, 0] = True                                        # the pooled position is always a row of the packed stream
    dout = dout * keep.reshape(-1, 1).to(dtype)              # nothing downstream reads the dropped rows
    drop = (_rng_words(B + S), P_DROP, 33) if dropout else None
    ref = _reference(qkv, mask, dout, B, S, H, _drop_probs(ops, B, H, S, drop))
    qkv_p, dout_p = ops.pack_rows(qkv, plan, 3 * H * 64), ops.pack_rows(dout, plan, H * 64)
    out_p, lse_p = ops.attn_fwd_packed(qkv_p, plan, B, S, H, drop=drop)
    dqkv_p = ops.attn_bwd_packed(qkv_p, plan, out_p, dout_p, lse_p, B, S, H, drop=drop)
    torch.cuda.synchronize()
    _check_packed(f"packed {case} {'drop' if dropout else 'nodrop'} {dtype}", ops, plan, out_p, lse_p, dqkv_p, ref, B, S, H)


@DTYPES
@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("S", [40, 200, 300])
def test_packed_zero_length_sequences(ops, S, dropout, dtype):
    """A hand-built plan (no pooled row kept) with sequences of zero rows first, in the middle and last: those workgroups
    write nothing, read no key mask word, and the neighbours are exact.  The packed key mask holds exactly n_rows words."""
    B, H = 5, 2
    lens = [0, S, 0, max(1, S // 3), 0]
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
    qkv, dout = _dense_inputs(B, S, H, dtype, seed=S + 77)
    dout = dout * mask.reshape(-1, 1).to(dtype)
    drop = (_rng_words(S + 5), P_DROP, 45) if dropout else None
    ref = _reference(qkv, mask, dout, B, S, H, _drop_probs(ops, B, H, S, drop))
    idx = torch.from_numpy(dense).long().cuda()
    qkv_p = torch.zeros_like(qkv)
    qkv_p[:n] = qkv[idx]
    dout_p = torch.zeros_like(dout)
    dout_p[:n] = dout[idx]
    out_p, lse_p = ops.attn_fwd_packed(qkv_p, plan, B, S, H, drop=drop)
    dqkv_p = ops.attn_bwd_packed(qkv_p, plan, out_p, dout_p, lse_p, B, S, H, drop=drop)
    torch.cuda.synchronize()
    _check_packed(f"packed Sb=0 S={S} {'drop' if dropout else 'nodrop'} {dtype}", ops, plan, out_p, lse_p, dqkv_p, ref,
                  B, S, H)
    lse_c = lse_p.cpu().view(B, H, S)
    for b in (0, 2, 4):
        assert float(lse_c[b].abs().max()) == 0.0, f"lse of the empty sequence {b} written"


# ---------------------------------------------------------------------------------------------------------------------
# 3. grouped pairs (dual kernels) vs the reference
# ---------------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("text", ["masked", "packed", "packed_drop"])
@pytest.mark.parametrize("St", [1, 77, 128])
@pytest.mark.parametrize("Sa", [129, 197, 224, 240])
def test_grouped_pair_vs_reference(ops, Sa, St, text, dtype):
    """ViT-like problem A (unmasked) + text problem B in one grouped call, both orders, under onepass 2 / 1 / 0.
    Sa = 240 is refused by dual_pair: the separate launches."""
    Ba, Ha, Bt, Ht = 2, 3, 3, 2
    qa, da = _dense_inputs(Ba, Sa, Ha, dtype, seed=Sa)
    qt, dt = _dense_inputs(Bt, St, Ht, dtype, seed=1000 + St)
    lens = [St, max(1, St // 2), max(1, St - 1)]
    mask = _prefix_mask(Bt, St, lens)
    if St > 2:
        mask[2, 1] = 0                   # a hole: packed index != position from there on (the dropout position table)
    if text != "masked":                                     # packed: the dropped (padding) rows carry no gradient
        keep = (mask != 0).clone()
        keep[:, 0] = True
        dt = dt * keep.reshape(-1, 1).to(dtype)
    drop = (_rng_words(St + Sa), P_DROP, 17) if text == "packed_drop" else None
    ref_a = _reference(qa, None, da, Ba, Sa, Ha)
    ref_t = _reference(qt, mask, dt, Bt, St, Ht, _drop_probs(ops, Bt, Ht, St, drop))
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
            tag = f"grouped Sa={Sa} St={St} {text} {dtype} onepass={mode} {oname}"
            _check_all(tag + " A", pa["out"], pa["lse"], pa["dqkv"], ref_a, Ha)
            if text == "masked":
                _check_all(tag + " B", pt["out"], pt["lse"], pt["dqkv"], ref_t, Ht)
            else:
                _check_packed(tag + " B", ops, plan, pt["out"], pt["lse"], pt["dqkv"], ref_t, Bt, St, Ht)


# ---------------------------------------------------------------------------------------------------------------------
# 4. adversarial values
# ---------------------------------------------------------------------------------------------------------------------

def _adversarial(kind, B, S, H, dtype, seed):
    x = _randn((B * S, 3, H, 64), seed)
    if kind == "sharp":              # |score| up to ~60, rows near one-hot
        x[:, :2] *= 4.5
    elif kind == "rising":           # score rises ~5 (natural log units) per 32 keys: the running maximum moves on every sub-tile
        x[:, 0] = 1.0 + 0.3 * x[:, 0]
        j = torch.arange(S, device="cuda", dtype=F32).repeat(B)
        x[:, 1] = (5.0 / 256.0) * j[:, None, None] + 0.3 * x[:, 1]
    elif kind == "offset":           # V = offset + noise: delta = rowsum(dO o O) is a difference of large terms
        # delta is summed from the STORED 16-bit O, so its error grows with offset * ulp(offset): the offset is scaled to the
        # storage type (8 in fp16, 2 in bf16: the same rounding step 2^-7 in both, 8 resp. 2 standard deviations of V)
        x[:, 2] += 8.0 if dtype == torch.float16 else 2.0
    else:
        raise ValueError(kind)
    return x.reshape(B * S, 3 * H * 64).to(dtype), _randn((B * S, H * 64), seed + 1).to(dtype)


@DTYPES
@pytest.mark.parametrize("kind", ["sharp", "rising", "offset"])
@pytest.mark.parametrize("S", [64, 197, 577])
def test_adversarial_scores(ops, S, kind, dtype):
    B, H = 2, 3
    qkv, dout = _adversarial(kind, B, S, H, dtype, seed=S * 7 + len(kind))
    ref = _reference(qkv, None, dout, B, S, H)
    if kind == "sharp":
        assert float(ref[1].max()) > 30.0
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
    qkv, dout = _dense_inputs(B, S, H, dtype, seed=S + 300)
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
