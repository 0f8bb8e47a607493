"""The sampled decode step (mh_sample_step), restated for the sampling tests (not a test module).

``uniform``          the draw's uniform of (seed, row, column) in Python integers: exact.
``tempered``         the logits after the processors (tests/logits_process_restatement.process in float32: one multiply or divide per
                     value, exact) and one float32 division by the float32 temperature: bit for bit what the kernel filters.
``kept_set``         the tokens that survive top-k and top-p, in float64 over those float32 values, by the rule include/memehip.h
                     states: top-k keeps every value >= the k-th largest (ties included); top-p keeps a survivor iff the mass of the
                     survivors with a strictly larger value is < top_p * Z (equal values share their fate).  A -inf value (a banned
                     token) is never kept: its probability is exactly 0.
``draw_interval``    each kept token's share [lo, hi) of the kept mass, in ascending index order, in float64.
``top_p_margin``     the smallest |mass above - top_p * Z| / Z over the survivors that have anything above them.  The tests demand
                     2^-15 of it, so that no kept / dropped decision hangs on rounding.  The survivor with nothing above it is left
                     out: an empty sum is 0 in every arithmetic, so it is kept for every top_p > 0 without any error (that is what
                     lets top_p = 1e-6 be a case at all).
``hf_warpers``       transformers' own TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper.

Settings travel as dicts: the processors' as in logits_process_restatement, the sampling ones as
``dict(temperature=1.0, top_k=0, top_p=1.0)`` (missing keys are neutral).  The C ABI carries temperature and top_p as floats, so the
restatement rounds them to float32 first."""
import numpy as np
import torch
from transformers import LogitsProcessorList, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

from logits_process_restatement import process

SAMPLING_NEUTRAL = dict(temperature=1.0, top_k=0, top_p=1.0)
M32 = 0xffffffff
D = 2.0 ** -15          # twice the kernel's summation bound of 2^-16 (it also covers expf and the x - max subtraction)


def sampling(**kw):
    unknown = set(kw) - set(SAMPLING_NEUTRAL)
    assert not unknown, unknown
    return dict(SAMPLING_NEUTRAL, **kw)


def hash32(x):
    """the counter hash of the dropout sites (lowbias32), on a Python int"""
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def seed_words(seed):
    return seed & M32, (seed >> 32) & M32


def uniform(seed, row, col):
    """(h >> 8) * 2^-24 with h = hash(hash(hash(hash(seed_lo ^ 0x9E3779B9) + seed_hi) + row) + col): exact in a double and a float"""
    lo, hi = seed_words(seed)
    h = hash32(lo ^ 0x9E3779B9)
    h = hash32(h + hi)
    h = hash32(h + row)
    h = hash32(h + col)
    return (h >> 8) / 16777216.0


def tempered(logits, hist, P, eos, proc, samp):
    """float32 [R, V]: processors, then / temperature"""
    s = sampling(**samp)
    x = process(hist, logits.float(), P, eos, proc)
    if s["temperature"] != 1.0:
        x = x / torch.tensor(s["temperature"], dtype=torch.float32)
    return x + 0.0          # -0 -> +0: equal values, one representation


def _masses(x, s):
    """x float32 [V] -> (survivors of top-k [V] bool, e float64 [V] (0 outside), mass strictly above each value [V])"""
    xd = x.double()
    V = xd.numel()
    surv = torch.ones(V, dtype=torch.bool)
    k = s["top_k"]
    if 0 < k < V:
        surv = xd >= xd.sort(descending=True)[0][k - 1]
    m = xd[surv].max()
    e = torch.where(surv, torch.exp(xd - m), torch.zeros((), dtype=torch.float64))
    vals, inv = torch.unique(xd, return_inverse=True)              # ascending
    per_val = torch.zeros(len(vals), dtype=torch.float64).index_add_(0, inv, e)
    above_val = per_val.flip(0).cumsum(0).flip(0) - per_val        # mass of the strictly larger values
    return surv, e, above_val[inv]


def kept_set(logits, hist, P, eos, proc, samp):
    """bool [R, V]"""
    s = sampling(**samp)
    x = tempered(logits, hist, P, eos, proc, s)
    out = torch.zeros(x.shape, dtype=torch.bool)
    p = float(np.float32(s["top_p"]))
    for r in range(x.shape[0]):
        surv, e, above = _masses(x[r], s)
        keep = surv & torch.isfinite(x[r])
        if p < 1.0:
            keep &= above < p * e.sum()
        out[r] = keep
    return out


def top_p_margin(logits, hist, P, eos, proc, samp):
    """min over rows and over survivors with a non-empty set above them of |mass above - top_p Z| / Z (inf without top-p)"""
    s = sampling(**samp)
    p = float(np.float32(s["top_p"]))
    if p >= 1.0:
        return float("inf")
    x = tempered(logits, hist, P, eos, proc, s)
    worst = float("inf")
    for r in range(x.shape[0]):
        surv, e, above = _masses(x[r], s)
        Z = e.sum()
        sel = surv & torch.isfinite(x[r]) & (above > 0)
        if sel.any():
            worst = min(worst, float(((above[sel] - p * Z).abs() / Z).min()))
    return worst


def draw_interval(logits, hist, P, eos, proc, samp):
    """(lo, hi) float64 [R, V]: kept token i is drawn for lo[i] <= u < hi[i]; unkept tokens hold nan"""
    s = sampling(**samp)
    x = tempered(logits, hist, P, eos, proc, s)
    kept = kept_set(logits, hist, P, eos, proc, s)
    lo = torch.full(x.shape, float("nan"), dtype=torch.float64)
    hi = lo.clone()
    for r in range(x.shape[0]):
        xd = x[r].double()
        e = torch.where(kept[r], torch.exp(xd - xd[kept[r]].max()), torch.zeros((), dtype=torch.float64))
        c = e.cumsum(0) / e.sum()
        hi[r][kept[r]] = c[kept[r]]
        lo[r][kept[r]] = (c - e / e.sum())[kept[r]]
    return lo, hi


def hf_warpers(samp):
    s = sampling(**samp)
    w = LogitsProcessorList()
    if s["temperature"] != 1.0:
        w.append(TemperatureLogitsWarper(float(s["temperature"])))
    if s["top_k"] > 0:
        w.append(TopKLogitsWarper(top_k=s["top_k"], min_tokens_to_keep=1))
    if s["top_p"] < 1.0:
        w.append(TopPLogitsWarper(top_p=float(s["top_p"]), min_tokens_to_keep=1))
    return w


def check_draw(what, tok, u, kept, lo, hi):
    """token in the kept set, and lo - D <= u < hi + D for its interval (every row)"""
    for r, t in enumerate(tok.tolist()):
        assert kept[r, t], (what, r, t, "the drawn token is not in the restated kept set")
        assert float(lo[r, t]) - D <= u[r] < float(hi[r, t]) + D, (what, r, t, u[r], float(lo[r, t]), float(hi[r, t]))
