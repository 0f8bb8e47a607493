"""The autoregressive decode kernels of csrc/decode.hip against one plain reference: float64 torch on the CPU, computed from the same
16-bit (or f32) tensors the kernels read, rounded to 16 bits where a kernel stores 16 bits.

  case                                   kernel / path
  ----------------------------------------------------------------------------------------------------------------------------
  attn_decode cross / self               attn_decode_kernel + attn_decode_combine_kernel: nsplit forced to 1 2 3 7 22 64 and
                                           decode_splits' own choice, T in {1 31 32 33 63 64 65 100 577 2048} (nsplit 64 at T 33:
                                           62 of 64 splits own no key); ldq = 3 H 64 (the captioner's fused qkv rows) in both
                                           forms; ldo > H 64 with NaN in the gap; a cache of capacity > T with ld_t > H 64 and a
                                           non-dense ld_b; the self form at t = 0, chunk - 1, chunk, chunk + 1, cap - 1 (slot t
                                           owned by a split other than 0) and t >= cap (nothing stored, keys 0..cap-1 attend)
  attn_decode scores <kind>              scaled scores to +-200, one dominant key, all keys equal (out = mean of V), V near the
                                           16-bit maximum
  attn_decode determinism / host         the same nsplit bit-identical run to run; ld % 8, nsplit > 64, no workspace rejected
  greedy argmax V<v>                     greedy_step_kernel: V in {1 3 4 5 1023 1024 1025 30524}, columns [V, ldl) holding +inf /
                                           NaN / 1e30, ties inside a wave, across the 4 waves, across the 1024-column passes and
                                           at 0 / V-1, all -inf rows, NaN rows (torch.argmax: first NaN)
  greedy trajectory B<b>                 B in {1 64 300 1024} over many steps against a Python replay of transformers' greedy
                                           bookkeeping: pad after eos, rows finishing together, eos == pad, prompt_len 1 / 2 / 5,
                                           the last column of out_ids reached; the same sequence replayed from a captured graph
  decode_embed D<d>                      decode_embed_kernel: D in {8 64 255 256 257 768 1024 2048} (2049 rejected), B to 512,
                                           |mean| / std ~ 1e3, eps 1e-12 and 1e-5, ids and t outside their tables clamped

Bars (EPS32 = 2^-24, TOL_SUM = 1e-5, ulp = the 16-bit ulp of the reference):
  * attention: a score q.k / 8 summed in f32 is within ds = TOL_SUM x max_j sum_i |q_i k_ji| / 8; scores moved by <= ds move
    every softmax weight by a relative <= 2 ds, so |out - ref| <= 1 ulp + (2 ds + TOL_SUM) x sum_j p_j |v_j| (TOL_SUM covers the
    f32 weighted sums, the exp2 and the final division);
  * LayerNorm (decode_embed): x = f32(word + pos) exactly; the mean is within dm = TOL_SUM x sum|x| / D, rstd relative within
    dr = (TOL_SUM + (dm / std)^2) / 2 + 4 EPS32; |y - ref| <= 1 ulp + |gamma| rstd (dm + |x - mean| dr) + 32 EPS32 (|gamma
    (x - mean) rstd| + |beta|);
  * bit-exact: argmax indices (== torch.argmax), the whole greedy state, the cache slot written (== kv_new), and every byte a kernel
    must not write (NaN / random sentinels).
The fp16 and the bf16 library are both run.  Measured worst errors go through conftest.parity_log, as fractions of the bar.
"""
import ctypes as C
import math

import pytest
import torch

from conftest import parity_log

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64, I32, I64 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64
DTYPES = pytest.mark.parametrize("T16", [F16, BF16], ids=["fp16", "bf16"])
MANT = {F16: 10, BF16: 7}
EMIN = {F16: -14, BF16: -126}
EPS32 = 2.0 ** -24
TOL_SUM = 1e-5
FORM = 32 * EPS32
DEV = "cuda"


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_num_threads(16)
    import multimodal_propaganda_meme_classification_amd as m
    from multimodal_propaganda_meme_classification_amd import ops as _ops
    m.ops = _ops
    return m


def _name(T16):
    return "fp16" if T16 == F16 else "bf16"


def _lib(pkg, T16=BF16):
    return pkg._lib.load(_name(T16))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ulp(ref, T16):
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** EMIN[T16]))
    return torch.pow(2.0, (e - 1 - MANT[T16]).to(F64))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else I32).cpu()


# ---- mh_attn_decode ------------------------------------------------------------------------------------------------------------

NSPLITS = (1, 2, 3, 7, 22, 64, None)
TS = (1, 31, 32, 33, 63, 64, 65, 100, 577, 2048)


def _chunk(T, nsplit):
    return (-(-T // nsplit) + 31) // 32 * 32


class _Decode:
    """One attention-decode problem laid out as the captioner lays it out: q inside fused qkv rows (ldq = 3 H 64), out with a
    NaN-filled gap (ldo > H 64), k / v in a cache with ld_t > H 64, a non-dense ld_b and one spare row block behind the last row
    (every write outside slot t, inside or past the rows, shows as a changed sentinel)."""

    def __init__(self, T16, B, H, cap, seed, qscale=1.0, kv=None):
        g = torch.Generator().manual_seed(seed)
        self.T16, self.B, self.H, self.cap = T16, B, H, cap
        D = H * 64
        self.D, self.ldq, self.ldo = D, 3 * D, D + 24
        self.ld_t = D + 16
        self.ld_b = cap * self.ld_t + 40
        self.qkv = (torch.randn(B, 3 * D, generator=g) * qscale).to(T16)
        cache = torch.randn(2, (B + 1) * self.ld_b, generator=g)
        if kv is not None:                          # kv(k_view [B, cap, H, 64], v_view) fills the live slots
            kview, vview = self._view(cache[0]), self._view(cache[1])
            kv(kview, vview, g)
        self.cache = cache.to(T16)

    def _view(self, flat):
        return flat[:self.B * self.ld_b].view(self.B, self.ld_b)[:, :self.cap * self.ld_t].view(self.B, self.cap, self.ld_t)[:, :, :self.D] \
            .view(self.B, self.cap, self.H, 64)

    def run(self, pkg, T, nsplit, t=None):
        d = {"k": self.cache[0].cuda(), "v": self.cache[1].cuda(), "qkv": self.qkv.cuda()}
        out = torch.full((self.B * self.ldo,), float("nan"), dtype=self.T16, device=DEV)
        td = None if t is None else torch.tensor([t], dtype=I32, device=DEV)
        kv_new = d["qkv"].view(-1)[self.D:] if t is not None else None
        pkg.ops.attn_decode(d["qkv"], d["k"], d["v"], out, self.B, self.H, T, self.ldq, self.ld_b, self.ld_t, self.ldo, t_dev=td,
                            kv_new=kv_new, ld_new=self.ldq, nsplit=nsplit)
        torch.cuda.synchronize()
        return out.cpu(), d["k"].cpu(), d["v"].cpu()

    def reference(self, T, t=None):
        """float64 softmax(q k^T / 8) v over the keys the kernel must attend -> (ref [B, H, 64], sum_j p_j |v_j|, ds)"""
        q = self.qkv[:, :self.D].to(F64).view(self.B, self.H, 64)
        k, v = self._view(self.cache[0]).to(F64), self._view(self.cache[1]).to(F64)
        n = T if t is None else min(t + 1, T)
        k, v = k[:, :n].clone(), v[:, :n].clone()
        if t is not None and t < T:                 # this step's k / v replace slot t
            k[:, t] = self.qkv[:, self.D:2 * self.D].to(F64).view(self.B, self.H, 64)
            v[:, t] = self.qkv[:, 2 * self.D:].to(F64).view(self.B, self.H, 64)
        s = torch.einsum("bhd,bthd->bht", q, k) / 8.0
        p = torch.softmax(s, -1)
        ref = torch.einsum("bht,bthd->bhd", p, v)
        wabs = torch.einsum("bht,bthd->bhd", p, v.abs())
        ds = TOL_SUM * torch.einsum("bhd,bthd->bht", q.abs(), k.abs()).amax(-1, keepdim=True) / 8.0
        return ref, wabs, ds

    def check(self, out, ref, wabs, ds, what):
        """-> worst error / bar; asserts the bar and that the gap between the output rows kept its NaN"""
        o = out.view(self.B, self.ldo)
        assert torch.isnan(o[:, self.D:].float()).all(), f"{what}: the gap [H 64, ldo) of out was written"
        got = o[:, :self.D].to(F64).view(self.B, self.H, 64)
        bar = _ulp(ref, self.T16) + (2 * ds + TOL_SUM) * wabs
        err = (got - ref).abs()
        assert torch.isfinite(got).all() and (err <= bar).all(), f"{what}: max err {float(err.max()):.3e}, worst err/bar {float((err / bar).max()):.3f}"
        return float((err / bar).max())


def _cache_untouched(prob, k, v, t):
    """every element of k / v except (b, slot t, :H*64) is unchanged, and slot t holds kv_new bit for bit"""
    for which, got, src in (("k", k, prob.cache[0]), ("v", v, prob.cache[1])):
        exp = src.clone()
        if t is not None and t < prob.cap:
            off = 1 if which == "k" else 2
            for b in range(prob.B):
                base = b * prob.ld_b + t * prob.ld_t
                exp[base:base + prob.D] = prob.qkv[b, off * prob.D:(off + 1) * prob.D]
        assert torch.equal(_bits(got), _bits(exp)), f"{which}: bytes outside slot t changed, or slot t != kv_new"


@DTYPES
def test_attn_decode_cross_sweep(pkg, T16):
    """cross form: every forced nsplit x every T; the same nsplit twice is bit-identical; all nsplit values within the bar"""
    B, H = 2, 3
    worst = 0.0
    for T in TS:
        prob = _Decode(T16, B, H, T + 5, seed=T)
        ref, wabs, ds = prob.reference(T)
        for ns in NSPLITS:
            out, k, v = prob.run(pkg, T, ns)
            worst = max(worst, prob.check(out, ref, wabs, ds, f"cross T={T} nsplit={ns}"))
            again, _, _ = prob.run(pkg, T, ns)
            assert torch.equal(_bits(out), _bits(again)), f"cross T={T} nsplit={ns}: not bit-identical run to run"
            _cache_untouched(prob, k, v, None)
    parity_log(f"[decode attn_decode cross {_name(T16)}] out {worst:.3e}")
    assert worst <= 1.0


@DTYPES
def test_attn_decode_self_sweep(pkg, T16):
    """self form: slot t at 0, chunk-1, chunk, chunk+1 and cap-1 of each forced split size (the owner of slot t is not split 0),
    the cache elsewhere untouched; t >= cap stores nothing and attends to the cached keys 0..cap-1"""
    B, H = 2, 2
    worst = 0.0
    for cap in (1, 33, 65, 577):
        prob = _Decode(T16, B, H, cap, seed=100 + cap)
        for ns in NSPLITS:
            nse = ns if ns is not None else pkg.ops.decode_splits(B, H, cap)
            ch = _chunk(cap, nse)
            for t in sorted({0, ch - 1, ch, ch + 1, cap - 1, cap, cap + 3}):
                if t < 0 or (t > cap - 1 and t not in (cap, cap + 3)):
                    continue
                ref, wabs, ds = prob.reference(cap, t)
                out, k, v = prob.run(pkg, cap, ns, t)
                worst = max(worst, prob.check(out, ref, wabs, ds, f"self cap={cap} nsplit={ns} t={t}"))
                _cache_untouched(prob, k, v, t)
    parity_log(f"[decode attn_decode self {_name(T16)}] out {worst:.3e}")
    assert worst <= 1.0


def _scores_large(kv_k, kv_v, g, q):
    c = 2 * torch.rand(kv_k.shape[:3], generator=g) - 1          # score_j = c_j |q|^2 / 8 = c_j x 200
    kv_k.copy_(c[..., None] * q[:, None] + 0.01 * torch.randn(kv_k.shape, generator=g))


@DTYPES
@pytest.mark.parametrize("kind", ["large", "dominant", "equal", "vmax"])
def test_attn_decode_adversarial_scores(pkg, T16, kind):
    B, H, cap = 2, 2, 577
    big = 0.99 * (65504.0 if T16 == F16 else 2.0 ** 110)    # bf16: the f32 accumulator sums up to cap |v|, which must stay below f32's maximum
    qscale = math.sqrt(1600.0 / 64) if kind == "large" else 1.0     # |q|^2 = 1600: q.q / 8 = 200
    g0 = torch.Generator().manual_seed(7)
    qkv = torch.randn(B, 3 * H * 64, generator=g0) * qscale
    q16 = qkv[:, :H * 64].to(T16).float().view(B, H, 64)

    def fill(k, v, g):
        if kind == "large":
            _scores_large(k, v, g, q16)
        elif kind == "dominant":
            k.mul_(0.1)
            k[:, 40] = q16 * 4.0                       # score ~ 4 |q|^2 / 8 ~ 32 above the rest
        elif kind == "equal":
            k.copy_(k[:, :1].clone().expand_as(k))
        else:
            v.copy_(big * (0.5 + 0.5 * torch.rand(v.shape, generator=g)) * torch.sign(torch.randn(v.shape, generator=g)))

    prob = _Decode(T16, B, H, cap, seed=11, kv=fill)
    prob.qkv = qkv.to(T16)
    worst = 0.0
    for T in (65, 577):
        ref, wabs, ds = prob.reference(T)
        if kind == "equal":
            mean_v = prob._view(prob.cache[1]).to(F64)[:, :T].mean(1)
            assert torch.allclose(ref, mean_v, rtol=1e-12, atol=1e-12)
        for ns in (1, 7, 64, None):
            out, _, _ = prob.run(pkg, T, ns)
            worst = max(worst, prob.check(out, ref, wabs, ds, f"{kind} T={T} nsplit={ns}"))
    parity_log(f"[decode attn_decode scores {kind} {_name(T16)}] out {worst:.3e}")
    assert worst <= 1.0


@DTYPES
def test_attn_decode_host_validation(pkg, T16):
    lib = _lib(pkg, T16)
    B, H, T = 1, 1, 64
    q = torch.zeros(3 * 64 * 2, dtype=T16, device=DEV)
    kv = torch.zeros(T * 64 + 64, dtype=T16, device=DEV)
    out = torch.zeros(128, dtype=T16, device=DEV)
    ws = torch.zeros(B * H * 64 * 66, dtype=F32, device=DEV)
    p = lambda t: t.data_ptr()

    def call(ldq=64, ld_t=64, ld_b=T * 64, ldo=64, ns=1, w=ws):
        return lib.mh_attn_decode(p(q), ldq, p(kv), p(kv), ld_b, ld_t, None, 0, None, T, p(out), ldo,
                                  None if w is None else p(w), ns, B, H, _st())
    assert call() == 0
    torch.cuda.synchronize()
    for kw in ({"ldq": 68}, {"ld_t": 60}, {"ld_b": T * 64 + 4}, {"ldo": 60}, {"ns": 65}, {"ns": 0}):
        assert call(**kw) != 0, kw
    assert call(ns=2, w=None) != 0
    assert call(ns=1, w=None) == 0                   # one split needs no workspace
    torch.cuda.synchronize()
    td = torch.zeros(1, dtype=I32, device=DEV)
    assert lib.mh_attn_decode(p(q), 64, p(kv), p(kv), T * 64, 64, None, 0, p(td), T, p(out), 64, None, 1, B, H, _st()) != 0  # no kv_new


# ---- mh_greedy_step ------------------------------------------------------------------------------------------------------------

def _argmax_rows(V, ldl, n_rows, seed):
    """logits [n_rows, ldl]: each row one tie / non-finite pattern; columns >= V hold +inf, NaN or 1e30"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_rows, ldl, generator=g)
    pads = (float("inf"), float("nan"), 1e30)
    for r in range(n_rows):
        x[r, V:] = pads[r % 3]
    def put(r, cols, val=50.0):
        for c in cols:
            if c < V:
                x[r, c] = val
    put(1, (4, 8))                          # lanes 1 and 2 of wave 0
    put(2, (1000, 768, 300))                # waves 3, 3, 1 (c = 4 tid): lowest index 300
    put(3, (1030, 6))                       # c and c + 1024: the second pass
    put(4, (0, V - 1))
    put(5, (V - 1,))
    x[6, :V] = float("-inf")
    put(7, (V - 1, V // 2, V // 3 + 1), float("nan"))
    x[8, :V] = float("nan")
    put(9, (V // 2 + 1, 2), float("inf"))
    put(10, (3,), float("-inf"))
    put(11, (1029, 1027, 2051, 5), 7.0)     # ties across passes and lanes
    return x


@pytest.mark.parametrize("V", [1, 3, 4, 5, 1023, 1024, 1025, 30524])
def test_greedy_argmax_edges(pkg, V):
    """one step: next_ids == torch.argmax over the first V columns (first maximum; NaN wins, first NaN; all -inf: 0)"""
    ldl = (V + 3) // 4 * 4 + 4
    rows = 12
    x = _argmax_rows(V, ldl, rows, seed=V)
    ref = torch.argmax(x[:, :V], dim=1)
    logits = x.cuda()
    out_ids = torch.zeros((rows, 2), dtype=I64, device=DEV)
    nxt = torch.full((rows,), -7, dtype=I64, device=DEV)
    fin = torch.zeros(rows, dtype=I32, device=DEV)
    state = torch.zeros(4, dtype=I32, device=DEV)
    pkg.ops.greedy_step(logits, V, out_ids, nxt, fin, state, 1, -1, 0)
    got = nxt.cpu()
    assert torch.equal(got, ref), (got, ref)
    assert torch.equal(out_ids.cpu()[:, 1], ref) and torch.equal(out_ids.cpu()[:, 0], torch.zeros(rows, dtype=I64))
    assert state.cpu().tolist() == [1, 0, 0, 0] and not fin.cpu().any()
    parity_log(f"[decode greedy argmax V{V}] next_ids == torch.argmax ({rows} tie / non-finite rows)")


def _replay(out_ids, fin, state, logits, V, P, eos, pad):
    """transformers' greedy bookkeeping for one step, on CPU tensors, in place"""
    B, ld_out = out_ids.shape
    t = int(state[0])
    col = t + 1
    nxt = None
    if col < ld_out:
        nxt = torch.empty(B, dtype=I64)
        am = torch.argmax(logits[:, :V], dim=1)
        for b in range(B):
            if col < P:
                tok = int(out_ids[b, col])
            elif fin[b]:
                tok = pad
            else:
                tok = int(am[b])
                if tok == eos:
                    fin[b] = 1
                    state[2] += 1
                    if int(state[2]) == B:
                        state[3] = col + 1
            out_ids[b, col] = tok
            nxt[b] = tok
    state[0] = t + 1
    return nxt


def _step_logits(B, V, ldl, eos, step, seed):
    g = torch.Generator().manual_seed(seed * 1000 + step)
    x = torch.randn(B, ldl, generator=g)
    x[:, V:] = float("nan")
    hit = torch.rand(B, generator=g) < 0.1 + 0.05 * step      # a growing share of the rows picks eos (many finish together)
    x[hit, eos] = 100.0
    if step % 3 == 1:                               # ties with eos: the lower index wins
        x[hit, 0] = 100.0
    return x


@pytest.mark.parametrize("B,V,P,eos,pad", [(1, 5, 1, 2, 0), (64, 30524, 2, 102, 0), (300, 1025, 5, 1024, 1024), (1024, 1023, 1, 7, 0)],
                         ids=["B1", "B64", "B300_eos_is_pad", "B1024"])
def test_greedy_trajectory(pkg, B, V, P, eos, pad):
    """many consecutive steps: out_ids / finished / state / next_ids after every step == the Python replay; the last steps run
    past ld_out; the same sequence replayed from one captured graph == the eager run"""
    ldl = (V + 3) // 4 * 4
    steps = 14
    ld_out = P + steps - 3
    g = torch.Generator().manual_seed(B)
    prompt = torch.randint(0, V, (B, P), generator=g)
    t0 = 0 if P > 1 else P - 1                       # P > 1: walk the prompt one token at a time, as the captioner does
    out0 = torch.zeros((B, ld_out), dtype=I64)
    out0[:, :P] = prompt
    fin0 = torch.zeros(B, dtype=I32)
    state0 = torch.tensor([t0, 0, 0, 0], dtype=I32)
    if B > 1:
        fin0[B // 3] = 1                             # a row finished before the first step
        state0[2] = 1
    logs = [_step_logits(B, V, ldl, eos, s, B) for s in range(steps)]
    ref_out, ref_fin, ref_state = out0.clone(), fin0.clone(), state0.clone()

    def fresh():
        return out0.clone().cuda(), torch.zeros(B, dtype=I64, device=DEV), fin0.clone().cuda(), state0.clone().cuda()

    out_ids, nxt, fin, state = fresh()
    logits = torch.empty((B, ldl), device=DEV)
    trajectory = []
    for s in range(steps):
        logits.copy_(logs[s])
        pkg.ops.greedy_step(logits, V, out_ids, nxt, fin, state, P, eos, pad)
        rn = _replay(ref_out, ref_fin, ref_state, logs[s], V, P, eos, pad)
        torch.cuda.synchronize()
        assert torch.equal(out_ids.cpu(), ref_out), f"step {s}: out_ids"
        assert torch.equal(fin.cpu(), ref_fin), f"step {s}: finished"
        assert state.cpu().tolist() == ref_state.tolist(), f"step {s}: state {state.cpu().tolist()} != {ref_state.tolist()}"
        if rn is not None:
            assert torch.equal(nxt.cpu(), rn), f"step {s}: next_ids"
        trajectory.append((out_ids.cpu(), fin.cpu(), state.cpu(), nxt.cpu()))
    assert int(ref_state[2]) > int(state0[2])        # the run did finish rows

    out_ids, nxt, fin, state = fresh()
    logits.zero_()
    gr = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        wo, wn, wf, ws = fresh()                     # a warm-up call outside the graph, on scratch state
        pkg.ops.greedy_step(logits, V, wo, wn, wf, ws, P, eos, pad)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(gr):
        pkg.ops.greedy_step(logits, V, out_ids, nxt, fin, state, P, eos, pad)
    for s in range(steps):
        logits.copy_(logs[s])
        gr.replay()
        torch.cuda.synchronize()
        eo, ef, es, en = trajectory[s]
        assert torch.equal(out_ids.cpu(), eo) and torch.equal(fin.cpu(), ef) and torch.equal(state.cpu(), es), f"graph step {s}"
        if s + 1 + t0 < ld_out:
            assert torch.equal(nxt.cpu(), en), f"graph step {s}: next_ids"
    parity_log(f"[decode greedy trajectory B{B} V{V} P{P}] {steps} steps == Python replay, eager and graph")


def test_greedy_host_validation(pkg):
    lib = pkg._lib.load()
    lg = torch.zeros((2, 8), device=DEV)
    o = torch.zeros((2, 4), dtype=I64, device=DEV)
    n = torch.zeros(2, dtype=I64, device=DEV)
    f = torch.zeros(2, dtype=I32, device=DEV)
    s = torch.zeros(4, dtype=I32, device=DEV)
    p = lambda t: t.data_ptr()
    assert lib.mh_greedy_step(p(lg), 8, 9, 2, p(o), 4, p(n), p(f), p(s), 1, 1, 0, _st()) != 0      # V > ldl
    assert lib.mh_greedy_step(p(lg), 6, 5, 2, p(o), 4, p(n), p(f), p(s), 1, 1, 0, _st()) != 0      # ldl % 4
    assert lib.mh_greedy_step(p(lg), 8, 8, 2, p(o), 1, p(n), p(f), p(s), 1, 1, 0, _st()) != 0      # ld_out <= prompt_len
    assert lib.mh_greedy_step(p(lg), 8, 8, 2, p(o), 4, p(n), p(f), None, 1, 1, 0, _st()) != 0      # no state


# ---- mh_decode_embed -----------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("D", [8, 64, 255, 256, 257, 768, 1024, 2048])
def test_decode_embed(pkg, T16, D):
    V, P = 50, 20
    g = torch.Generator().manual_seed(D)
    word = torch.randn(V, D, generator=g)
    word[7] = 1e3 + torch.randn(D, generator=g)      # |mean| / std ~ 1e3
    word[8] = -1e3 + 0.5 * torch.randn(D, generator=g)
    pos = 0.3 * torch.randn(P, D, generator=g)
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    worst = 0.0
    for B, ids_list in ((3, [7, 8, 0]), (512, None)):
        ids = torch.randint(0, V, (B,), generator=g) if ids_list is None else torch.tensor(ids_list)
        if ids_list is None:
            ids[:6] = torch.tensor([-5, V, V + 100, 7, 8, V - 1])
        for t in (0, P - 1, -3, P + 7, 5):
            for eps in (1e-12, 1e-5):
                y = torch.full((B, D), float("nan"), dtype=T16, device=DEV)
                td = torch.tensor([t], dtype=I32, device=DEV)
                pkg.ops.decode_embed(ids.cuda(), td, word.cuda(), pos.cuda(), gamma.cuda(), beta.cuda(), eps, y)
                got = y.cpu().to(F64)
                idc, tc = ids.clamp(0, V - 1), min(max(t, 0), P - 1)      # the clamps the header states
                x = (word[idc] + pos[tc]).to(F64)                         # f32 + f32 -> f32: exact as the kernel's sum
                mean = x.mean(1, keepdim=True)
                var = ((x - mean) ** 2).mean(1, keepdim=True)
                rstd = 1.0 / torch.sqrt(var + eps)
                ref = (x - mean) * rstd * gamma.to(F64) + beta.to(F64)
                dm = TOL_SUM * x.abs().sum(1, keepdim=True) / D
                dr = (TOL_SUM + (dm / var.sqrt()) ** 2) / 2 + 4 * EPS32
                ga = gamma.to(F64).abs()
                bar = _ulp(ref, T16) + ga * rstd * (dm + (x - mean).abs() * dr) + FORM * ((ref - beta.to(F64)).abs() + beta.to(F64).abs())
                err = (got - ref).abs()
                assert (err <= bar).all(), f"D={D} B={B} t={t} eps={eps}: worst err/bar {float((err / bar).max()):.3f}"
                worst = max(worst, float((err / bar).max()))
    lib = _lib(pkg, T16)
    p = lambda t: t.data_ptr()
    big = torch.zeros((1, 2049), device=DEV)
    yb = torch.zeros(2049, dtype=T16, device=DEV)
    i1 = torch.zeros(1, dtype=I64, device=DEV)
    t1 = torch.zeros(1, dtype=I32, device=DEV)
    assert lib.mh_decode_embed(p(i1), p(t1), p(big), p(big), p(big), p(big), p(yb), 1, 2049, 1, 1, C.c_float(1e-5), _st()) != 0
    parity_log(f"[decode decode_embed D{D} {_name(T16)}] y {worst:.3e}")
