"""The two attention checks of tests/test_attention_paths_gpu.py, validated without a GPU (tests/attention_restatement.py):

  * the tied-score case is exactly representable in fp16 and bf16 -- out, dQ, dK, dV and the 16-bit MFMA operands P o M and dS --
    at every shape the GPU tests run it, with and without a 0 / 2 dropout multiplier, and has the structure it promises (P is
    1/n on 1, 2 or 4 keys, the rest >= 100 below; null and masked keys get no gradient; dQ and dK are non-trivial);
  * the float32 emulation of the kernels stays inside the derived per-tensor bound on the random and adversarial inputs of the
    GPU tests (the same laws and seeds, drawn on the CPU) at S = 64 / 197 / 577; the worst error / bound ratio is logged.  On
    the `offset` inputs the delta term is the largest term of the dQ bound: it is what that case is there to stress."""
import pytest
import torch

import attention_restatement as R
from conftest import parity_log

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
TENSORS = ("out", "lse", "dQ", "dK", "dV")


def _mult(B, H, S, p, seed):
    """dropout multipliers 0 or 1 / (1 - p), [B, H, S, S]"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B, H, S, S), generator=g) >= p).to(torch.float64) / (1.0 - p)


@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("shape", list(R.tied_shapes()), ids=lambda s: s[0].replace(" ", "_"))
def test_tied_case_is_exact(shape, dropout):
    tag, B, S, H, mask = shape
    qkv, dout = R.tied_case(B, S, H, mask, R.tied_seed(B, S, H))
    m = None if mask is None else torch.from_numpy(mask)
    r = R.reference(qkv, dout, B, S, H, m, _mult(B, H, S, 0.5, S) if dropout else None, flush=True)
    for dtype in (torch.float16, torch.bfloat16):
        for name in ("q", "k", "v", "do", "PM", "dS", "O", "dQ", "dK", "dV"):
            assert R.representable(getattr(r, name).contiguous(), dtype), f"{tag}: {name} is not exact in {dtype}"
    # structure: every probability is 0, 1, 1/2 or 1/4 and the runner-up is >= 100 below the tie
    assert bool(((r.P == 0) | (r.P == 1) | (r.P == 0.5) | (r.P == 0.25)).all()), tag
    live_q = ~r.dead.expand(B, H, S, 1)
    top = r.s.max(-1, keepdim=True).values
    below = r.s.masked_fill(r.s == top, -float("inf")).max(-1, keepdim=True).values
    assert bool(((top - below >= 100) | ~live_q).all()), tag
    # keys nobody attends to (null, masked) get exactly no gradient
    unseen = (r.P.sum(-2) == 0)[..., None]
    assert float((r.dK * unseen).abs().max()) == 0.0 and float((r.dV * unseen).abs().max()) == 0.0, tag
    if S >= 31 and not bool(r.dead.all()):
        assert float((r.dQ != 0).double().mean()) > 0.05 and float((r.dK != 0).double().mean()) > 0.03, tag


def _inside(tag, qkv, dout, B, S, H, dtype, mask=None, pm=None, parts=False):
    r = R.reference(qkv, dout, B, S, H, mask, pm)
    b = R.bounds(r, dtype, parts=parts)
    e = R.emulate(qkv, dout, B, S, H, dtype, mask, pm)
    worst = {n: R.ratio(e[n], getattr(r, "O" if n == "out" else n), b[n]) for n in TENSORS}
    parity_log(f"[attention bound, float32 emulation, {tag} {dtype}] worst error / bound " +
               " ".join(f"{n} {worst[n]:.3f}" for n in TENSORS))
    for n in TENSORS:
        assert worst[n] <= 1.0, f"{tag}: the emulation's {n} is {worst[n]:.3f} of its bound"
    return b


@DTYPES
@pytest.mark.parametrize("drop", [None, 0.1], ids=["nodrop", "drop"])
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("S", [64, 197, 577])
def test_emulation_inside_bound_random(S, masked, drop, dtype):
    B, H = 3, 2
    qkv, dout = R.dense_inputs(B, S, H, dtype, S, "cpu")
    mask = torch.from_numpy(R.prefix_mask(S, [S, 0, max(1, (S + 1) // 2)])) if masked else None     # one row with no key
    pm = _mult(B, H, S, drop, S + 1) if drop else None
    _inside(f"random S={S} {'masked' if masked else 'unmasked'} {'drop' if drop else 'nodrop'}", qkv, dout, B, S, H, dtype,
            mask, pm)


@DTYPES
@pytest.mark.parametrize("kind", ["sharp", "rising", "offset"])
@pytest.mark.parametrize("S", [64, 197, 577])
def test_emulation_inside_bound_adversarial(S, kind, dtype):
    B, H = 2, 3
    qkv, dout = R.adversarial(kind, B, S, H, dtype, S * 7 + len(kind), "cpu")
    b = _inside(f"adversarial {kind} S={S}", qkv, dout, B, S, H, dtype, parts=True)
    if kind == "offset":
        p = b["dQ_parts"]
        assert max(p, key=p.get) == "delta", p


@DTYPES
def test_emulation_reproduces_the_tied_case(dtype):
    """the emulation has the kernels' rounding points, so it reproduces the exact case bit for bit, dropout twin included"""
    B, S, H = 3, 197, 2
    mask = R.prefix_mask(S, R.lens(S))
    qkv, dout = R.tied_case(B, S, H, mask, R.tied_seed(B, S, H))
    for pm in (None, _mult(B, H, S, 0.5, 3)):
        r = R.reference(qkv, dout, B, S, H, torch.from_numpy(mask), pm, flush=True)
        e = R.emulate(qkv, dout, B, S, H, dtype, torch.from_numpy(mask), pm)
        for n in ("out", "dQ", "dK", "dV"):
            assert torch.equal(e[n].to(torch.float64), getattr(r, "O" if n == "out" else n)), n
