"""Attention (csrc/attention.hip), restated for the attention tests (not a test module; no GPU code).

``tied_case``   inputs whose attention is exact in fp16 AND bf16.  Per (batch row, head), over the L live keys (all S, or the
                positions the key mask keeps): rank r sits at live[(37 r) mod L] when gcd(37, L) = 1, else live[r]; runs of
                consecutive ranks form at most 64 groups -- one of size 1, one of size 2, the others of size 4, a remainder of
                1 / 2 / 3 ranks as [1] / [2] / [2, 1]; past 248 grouped keys the live keys are null keys.  Class c (= group c)
                owns dimension c % 32 with sign + (c < 32) or - : q and k carry 32 * sign there and 0 in the other 31; a null key
                carries 0 in all 32.  Dims 32..47 are integer noise in [-2, 2] in k only, dims 48..63 in q only, so the noise
                never reaches a score: q.k / 8 is 128 inside a class, -128 against the opposite sign, 0 otherwise.  A position
                without a group (null or masked) is still a query, of class position % n_groups.  V is dense in {-1, 0, 1};
                dO has 8 entries of +-1 per (row, head).  Then P is 1/n on the query's n tied keys and 0 elsewhere (the other
                keys are >= 128 below: exp2(-184) = 0 in float32 too), O, dP, delta, dS are small dyadic rationals, and out, dQ,
                dK, dV are representable in both 16-bit types (``representable`` checks that; tests/test_attention_bounds.py
                asserts it at every shape the GPU tests use).  dK and dV of null and masked keys are exactly 0.
``reference``   float64 attention with every intermediate (no autograd): s = q k^T / 8 + (1 - mask) finfo(float32).min,
                P = softmax, PM = P o M (M the dropout multipliers or 1), O = PM V, dP = (dO V^T) o M, delta = rowsum(dO o O),
                dS = P o (dP - delta), dQ = dS K / 8, dK = dS^T Q / 8, dV = PM^T dO.  A batch row whose key mask is all zeros
                has P = 0 (out = 0, lse = -inf, no gradient: include/memehip.h).  flush=True, for the tied case, drops the
                probabilities below float32's smallest subnormal (e^-128 is still 2.6e-56 in float64).
``bounds``      per-element first-order error bounds of the kernels' arithmetic, per tensor, from those intermediates (below).
``emulate``     the kernels' algorithm in float32 with the 16-bit roundings where the kernels have them; the arbiter of
                ``bounds`` on a machine without a GPU.

The bound.  u = 2^-11 (fp16) or 2^-8 (bf16) is the unit roundoff of the storage type, f = 2^-24 that of float32, t = 2^-25 (fp16)
or 2^-134 (bf16) half the smallest subnormal (the absolute rounding error below the normal range: gradual underflow of a 16-bit MFMA
operand or of a stored value -- a term the relative u |x| alone lacks; it shows on the `sharp` inputs, whose P are mostly < 2^-14).
r(x) = max(u |x|, t) is one rounding of x to the storage type.  phi = 2^-126 is the absolute error of a float32 probability under the
normal range: v_exp_f32 returns 0 there instead of a subnormal (a second term the issue's count lacked: the `rising` inputs at
S = 577 have P down to 2^-150 and whole dV rows summed from such values; the kernels' dV was at 2.4 of a bound without it,
and so is the emulation once its exp2 flushes).  rP_ij = r(PM_ij) + phi M_ij is then the error of the P o M operand.
A_ij = sum_d |q_id k_jd| / 8.  One term per rounding in
attn_fwd_body / attn_bwd_dq_body / attn_bwd_dkv_body / attn_bwd_onepass_body (the dual and merged kernels call the same bodies):

  exponent   eta_ij = f (64 A_ij + 3 |s_ij| + 4 |lse_i| + 4): the float32 MFMA sum of 64 products (64 f A), the multiply by
             c = log2(e) / 8 and c's own rounding (2 f |s|), the key-bias add (f |s|), the subtraction of m or of lse * log2(e)
             with lse's two constant multiplies and its float32 store (4 f |lse|), v_exp_f32 / v_log_f32 at one ulp each and the
             rounding of log2(l) (4 f).  exp turns an absolute exponent error into a relative error of P: eps_ij = eta_ij.
  out        E_O = r(O) + sum_j (rP_ij + (eps_ij + 64 f) PM_ij) |v_jd| + (max_j eps_ij + S f) |O|: the store; P o M rounded
             to the PV operand, its exponent error, the float32 sum over the keys (64 f: one MFMA accumulates 64 keys of a tile
             before the next tile's partial sums join); the normaliser l (its terms' exponent errors, and -- a term the issue's
             count lacked -- its own float32 sum over S keys, S f).
  lse        max_j eta_ij + 4 f (1 + |lse_i|).
  dV         r(dV) + sum_i (rP_ij + (eps_ij + S f) PM_ij) |dO_id|.
  delta      D_i = sum_d |dO_id| E_O[i, d] + 64 f sum_d |dO_id O_id|  (summed in float32 from the STORED 16-bit O).
  dS         e_ij = P_ij D_i + r(dS_ij) + phi |dP_ij - delta_i| + eps_ij |dS_ij| + 64 f P_ij M_ij sum_d |dO_id v_jd|.
  dQ         r(dQ) + (1/8) sum_j (e_ij + S f |dS_ij|) |k_jd|        dK   r(dK) + (1/8) sum_i (e_ij + S f |dS_ij|) |q_id|.

The whole bound is doubled once for the second-order terms; nothing else is slack.  Where the bound is 0 (masked and null keys,
rows with no key) the kernels must write exactly 0."""
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
F = 2.0 ** -24
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}
LOG2E = 1.4426950408889634
PHI = 2.0 ** -126
SECOND_ORDER = 2.0


# ---------------------------------------------------------------------------------------------------------------------
# the tied-score case
# ---------------------------------------------------------------------------------------------------------------------

def group_sizes(L):
    """sizes of the tie groups over L live keys (at most 64 groups, at most 248 grouped keys)"""
    if L <= 2:
        return [L] if L > 0 else []
    rest = min(L, 248) - 3
    return [1, 2] + [4] * (rest // 4) + {0: [], 1: [1], 2: [2], 3: [2, 1]}[rest % 4]


def _classes(S, live):
    """(class of every position as a query, class of every position as a key or -1 for a null key, number of groups)"""
    L = len(live)
    sizes = group_sizes(L)
    ng, grouped = len(sizes), sum(sizes)
    order = live[(37 * np.arange(L)) % L] if L > 0 and math.gcd(37, L) == 1 else live
    qc = np.arange(S) % max(ng, 1)
    kc = qc.copy()                       # a masked key's class is never seen: its score is finfo.min
    kc[live] = -1
    gid = np.repeat(np.arange(ng), sizes)
    qc[order[:grouped]] = gid
    kc[order[:grouped]] = gid
    return qc, kc, ng


def tied_case(B, S, H, mask=None, seed=0):
    """float64 qkv [B*S, 3*H*64] and dout [B*S, H*64] of integers (exact in fp16 and bf16); mask: [B, S] of 0 / 1 or None"""
    g = np.random.default_rng(seed)
    q = np.zeros((B, S, H, 64))
    k = np.zeros((B, S, H, 64))
    m = None if mask is None else np.asarray(mask).reshape(B, S)
    for b in range(B):
        live = np.arange(S) if m is None else np.flatnonzero(m[b])
        qc, kc, _ = _classes(S, live)
        for x, cls in ((q, qc), (k, kc)):
            at = np.flatnonzero(cls >= 0)
            x[b, at, :, cls[at] % 32] = np.where(cls[at] < 32, 32.0, -32.0)[:, None]
    k[..., 32:48] = g.integers(-2, 3, (B, S, H, 16))
    q[..., 48:64] = g.integers(-2, 3, (B, S, H, 16))
    v = g.integers(-1, 2, (B, S, H, 64)).astype(np.float64)
    dout = np.zeros((B, S, H, 64))
    at = np.argsort(g.random((B, S, H, 64)), -1)[..., :8]
    np.put_along_axis(dout, at, g.choice([-1.0, 1.0], at.shape), -1)
    qkv = np.stack([q, k, v], 2).reshape(B * S, 3 * H * 64)
    return torch.from_numpy(qkv), torch.from_numpy(dout.reshape(B * S, H * 64))


def representable(x, dtype):
    """every element of the float64 tensor survives the round trip through dtype"""
    return torch.equal(x.to(dtype).to(F64), x)


# ---------------------------------------------------------------------------------------------------------------------
# the random and adversarial inputs of tests/test_attention_paths_gpu.py (on any device: the CPU tests draw the same laws)
# ---------------------------------------------------------------------------------------------------------------------

def randn(shape, seed, device, scale=1.0):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(shape, generator=g, device=device) * scale


def dense_inputs(B, S, H, dtype, seed, device):
    return randn((B * S, 3 * H * 64), seed, device).to(dtype), randn((B * S, H * 64), seed + 1, device).to(dtype)


def adversarial(kind, B, S, H, dtype, seed, device):
    x = randn((B * S, 3, H, 64), seed, device)
    if kind == "sharp":              # |score| up to ~60, rows near one-hot
        x[:, :2] *= 4.5
    elif kind == "rising":           # score rises ~5 (natural log units) per 32 keys: the running maximum moves on every sub-tile
        x[:, 0] = 1.0 + 0.3 * x[:, 0]
        j = torch.arange(S, device=device, dtype=F32).repeat(B)
        x[:, 1] = (5.0 / 256.0) * j[:, None, None] + 0.3 * x[:, 1]
    elif kind == "offset":           # V = offset + noise: delta = rowsum(dO o O) is a difference of large terms
        # delta is summed from the STORED 16-bit O, so its error grows with offset * ulp(offset): the offset is scaled to the
        # storage type (8 in fp16, 2 in bf16: the same rounding step 2^-7 in both, 8 resp. 2 standard deviations of V)
        x[:, 2] += 8.0 if dtype == torch.float16 else 2.0
    else:
        raise ValueError(kind)
    return x.reshape(B * S, 3 * H * 64).to(dtype), randn((B * S, H * 64), seed + 1, device).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference with its intermediates
# ---------------------------------------------------------------------------------------------------------------------

def heads(x, B, S, H):
    """[B*S, H*64] -> [B, H, S, 64]"""
    return x.view(B, S, H, 64).permute(0, 2, 1, 3)


def rows(x):
    """[B, H, S, 64] -> [B*S, H*64]"""
    B, H, S, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, H * 64)


def rows3(dq, dk, dv):
    """three [B, H, S, 64] -> dqkv [B*S, 3*H*64]"""
    return torch.stack([rows(dq), rows(dk), rows(dv)], 1).reshape(dq.shape[0] * dq.shape[2], -1)


class Ref:
    pass


def reference(qkv, dout, B, S, H, mask=None, pm=None, flush=False):
    """qkv [B*S, 3*H*64], dout [B*S, H*64], mask [B, S] or None, pm [B, H, S, S] dropout multipliers or None (any dtype, CPU).
    flush=True (the tied case) sets the probabilities below 2^-149 to 0: e^-128 is 2.6e-56 in float64 but nothing in float32,
    whose smallest subnormal that is; the tied P are then exactly 1/n and every result is an exact dyadic rational."""
    r = Ref()
    r.B, r.S, r.H = B, S, H
    x = qkv.detach().cpu().to(F64).view(B, S, 3, H, 64)
    r.q, r.k, r.v = x.permute(2, 0, 3, 1, 4)
    r.do = heads(dout.detach().cpu().to(F64), B, S, H)
    r.s = r.q @ r.k.transpose(-1, -2) / 8.0
    r.live = torch.ones(B, 1, 1, S, dtype=torch.bool)
    if mask is not None:
        m = mask.detach().cpu().to(F64).view(B, S)
        r.s = r.s + (1.0 - m)[:, None, None, :] * torch.finfo(F32).min
        r.live = (m != 0)[:, None, None, :]
    r.dead = ~r.live.any(-1, keepdim=True)                    # [B, 1, 1, 1]: no key to attend to
    r.P = torch.softmax(r.s, -1).masked_fill(r.dead, 0.0)
    if flush:
        r.P = r.P.masked_fill(r.P < 2.0 ** -149, 0.0)
    r.lse = torch.logsumexp(r.s, -1).masked_fill(r.dead[..., 0], -math.inf)
    r.M = torch.ones(()).to(F64) if pm is None else pm.to(F64)
    r.PM = r.P * r.M
    r.O = r.PM @ r.v
    r.dP = (r.do @ r.v.transpose(-1, -2)) * r.M
    r.delta = (r.do * r.O).sum(-1, keepdim=True)
    r.dS = r.P * (r.dP - r.delta)
    r.dQ = r.dS @ r.k / 8.0
    r.dK = r.dS.transpose(-1, -2) @ r.q / 8.0
    r.dV = r.PM.transpose(-1, -2) @ r.do
    return r


def bounds(r, dtype, parts=False, lse_only=False):
    """dict(out, lse, dQ, dK, dV): out, dQ, dK, dV as [B, H, S, 64], lse as [B, H, S]; the docstring's formulas, doubled once.
    parts=True adds 'dQ_parts': the mean share of each term of the dQ bound; lse_only=True (the tied case, whose other outputs
    are exact) returns the lse bound alone."""
    u, t, S = U[dtype], TINY[dtype], r.S
    rd = lambda x: (u * x.abs()).clamp_min(t) * (x != 0)      # one rounding to the storage type; an exact 0 stays 0
    av, ado = r.v.abs(), r.do.abs()
    lse_abs = r.lse.abs().masked_fill(r.dead[..., 0], 0.0)[..., None]
    A = r.q.abs() @ r.k.abs().transpose(-1, -2) / 8.0
    eta = F * (64.0 * A + 3.0 * r.s.abs() + 4.0 * lse_abs + 4.0)
    eta = eta.masked_fill(~r.live, 0.0).masked_fill(r.dead, 0.0)
    eps = eta
    eps_max = eps.max(-1, keepdim=True).values
    if lse_only:
        return dict(lse=SECOND_ORDER * (eps_max[..., 0] + 4 * F * (1.0 + lse_abs[..., 0])))
    phi = PHI * (r.live & ~r.dead)                            # only a key that is attended to has a probability to flush
    rP = rd(r.PM) + phi * r.M
    E_O = rd(r.O) + (rP + (eps + 64 * F) * r.PM) @ av + (eps_max + S * F) * r.O.abs()
    b_lse = eps_max[..., 0] + 4 * F * (1.0 + lse_abs[..., 0])
    b_dV = rd(r.dV) + (rP + (eps + S * F) * r.PM).transpose(-1, -2) @ ado
    D = (ado * E_O).sum(-1, keepdim=True) + 64 * F * (r.do * r.O).abs().sum(-1, keepdim=True)
    terms = dict(delta=r.P * D, ds_round=rd(r.dS) + phi * (r.dP - r.delta).abs(), exponent=eps * r.dS.abs(),
                 dp_sum=64 * F * r.P * r.M * (ado @ av.transpose(-1, -2)), dq_sum=S * F * r.dS.abs())
    e = sum(terms.values())
    b_dQ = rd(r.dQ) + e @ r.k.abs() / 8.0
    b_dK = rd(r.dK) + e.transpose(-1, -2) @ r.q.abs() / 8.0
    out = dict(out=SECOND_ORDER * E_O, lse=SECOND_ORDER * b_lse, dQ=SECOND_ORDER * b_dQ, dK=SECOND_ORDER * b_dK,
               dV=SECOND_ORDER * b_dV)
    if parts:
        p = {n: float((x @ r.k.abs() / 8.0).mean()) for n, x in terms.items()}
        p["store"] = float(rd(r.dQ).mean())
        out["dQ_parts"] = p
    return out


def ratio(got, want, bound):
    """worst |got - want| / bound over the finite references; an element whose bound is 0 must be exact (ratio inf otherwise)"""
    got, want, bound = got.detach().cpu().to(F64), want.to(F64), bound.to(F64)
    fin = torch.isfinite(want)
    if not torch.equal(got[~fin], want[~fin]) or not torch.isfinite(got[fin]).all():
        return math.inf
    err, b = (got[fin] - want[fin]).abs(), bound[fin]
    if bool(((b == 0) & (err > 0)).any()):
        return math.inf
    nz = b > 0
    return float((err[nz] / b[nz]).max()) if bool(nz.any()) else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' algorithm in float32, rounded to the 16-bit type where the kernels round
# ---------------------------------------------------------------------------------------------------------------------

def emulate(qkv, dout, B, S, H, dtype, mask=None, pm=None):
    """dict(out, lse, dQ, dK, dV) in the layout of ``bounds``.  float32 products and sums; P o M and dS rounded to dtype as MFMA
    operands; O, dQ, dK, dV rounded at the store; delta summed from the rounded O; the backward's P recomputed from the stored
    lse as exp2(s c - lse log2(e)); exp2 returns 0 below 2^-126 as v_exp_f32 does."""
    exp2 = lambda t: torch.where(t < -126.0, torch.zeros_like(t), torch.exp2(t))
    c = torch.tensor(0.125, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    x = qkv.detach().cpu().to(dtype).to(F32).view(B, S, 3, H, 64)
    q, k, v = x.permute(2, 0, 3, 1, 4)
    do = heads(dout.detach().cpu().to(dtype).to(F32), B, S, H)
    live = torch.ones(B, 1, 1, S, dtype=torch.bool) if mask is None else (mask.detach().cpu().view(B, S) != 0)[:, None, None, :]
    dead = ~live.any(-1, keepdim=True)
    M = torch.ones((), dtype=F32) if pm is None else pm.to(F32)
    rnd = lambda t: t.to(dtype).to(F32)
    s2 = (q @ k.transpose(-1, -2)) * c + (~live).to(F32) * -1.0e30
    m = s2.max(-1, keepdim=True).values
    p = exp2(s2 - m) * live
    l = p.sum(-1, keepdim=True)
    inv = torch.where(dead, torch.zeros_like(l), 1.0 / l)
    out = rnd((rnd(p * M) @ v) * inv)
    lse = ((m + torch.log2(l)) * torch.tensor(1.0 / LOG2E, dtype=F32)).masked_fill(dead, -math.inf)
    pb = exp2(s2 - lse * torch.tensor(LOG2E, dtype=F32)).masked_fill(dead, 0.0) * live
    delta = (do * out).sum(-1, keepdim=True)
    ds = rnd(pb * ((do @ v.transpose(-1, -2)) * M - delta))
    return dict(out=out, lse=lse[..., 0], dQ=rnd((ds @ k) * 0.125), dK=rnd((ds.transpose(-1, -2) @ q) * 0.125),
                dV=rnd(rnd(pb * M).transpose(-1, -2) @ do))


# ---------------------------------------------------------------------------------------------------------------------
# the masks and shapes of tests/test_attention_paths_gpu.py (numpy, so that the CPU tests walk the same ones)
# ---------------------------------------------------------------------------------------------------------------------

S_TABLE = [1, 31, 32, 33, 64, 65, 127, 128, 129, 160, 197, 223, 224, 225, 255, 256, 257, 300]
S_DROPOUT = [33, 128, 160, 224, 256, 257]
PACKED_CASES = ["edges", "holes", "s200", "s300"]


def lens(S):
    return [S, max(1, S - 1), max(1, (S + 1) // 2)]          # full, last key masked, half


def prefix_mask(S, ln):
    return (np.arange(S)[None] < np.array(ln)[:, None]).astype(np.int64)


def packed_mask(case):
    """[B, S] int64 masks; empty rows are all zeros"""
    if case == "edges":                      # empty first / middle / last, one token, the 32 / 64 boundaries
        S, ln = 80, [0, 1, 31, 0, 32, 33, 64, 65, 0]
        m = np.arange(S)[None] < np.array(ln)[:, None]
    elif case == "holes":
        S = 96
        g = np.random.default_rng(7)
        m = g.random((5, S)) < 0.5
        m[0, 0] = m[2, 0] = True
        m[1, 0] = False                      # the pooled row (position 0) is kept as a query but is no key
        m[3] = False                         # empty
        m[4, 40:] = False
    elif case == "s200":
        S, ln = 200, [200, 0, 129, 161]
        m = np.arange(S)[None] < np.array(ln)[:, None]
    elif case == "s300":
        S = 300
        g = np.random.default_rng(9)
        m = np.arange(S)[None] < np.array([300, 1, 0, 257])[:, None]
        m[0] &= g.random(S) < 0.7
        m[0, 0] = True
    else:
        raise ValueError(case)
    return m.astype(np.int64)


def zero_length_lens(S):
    return [0, S, 0, max(1, S // 3), 0]


def text_mask(St):
    """the text problem of the grouped pairs: three prefix lengths and a hole"""
    m = prefix_mask(St, [St, max(1, St // 2), max(1, St - 1)])
    if St > 2:
        m[2, 1] = 0                      # a hole: packed index != position from there on (the dropout position table)
    return m


def tied_seed(B, S, H):
    return 7919 * B + 31 * H + S


def tied_shapes():
    """(tag, B, S, H, mask or None) of every tied-score case the GPU tests run"""
    for S in S_TABLE + [577]:
        yield f"dense S={S}", 3, S, 2, None
        yield f"dense S={S} masked", 3, S, 2, prefix_mask(S, lens(S))
    for case in PACKED_CASES:
        m = packed_mask(case)
        yield f"packed {case}", m.shape[0], m.shape[1], 2, m
    for S in (40, 200, 300):
        yield f"packed Sb=0 S={S}", 5, S, 2, prefix_mask(S, zero_length_lens(S))
    for Sa in (129, 197, 224, 240):
        yield f"grouped A Sa={Sa}", 2, Sa, 3, None
    for St in (1, 77, 128):
        yield f"grouped B St={St}", 3, St, 2, text_mask(St)
    yield "geometry BERT-base", 2, 197, 12, None
    yield "geometry ViT-L", 1, 577, 16, None
