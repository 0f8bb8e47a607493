"""The fine-tune step on the MI355X, every gradient row against float64 by the derived bars of tests/step_restatement.py, and the
optimizer's wiring element by element.

For every case x {fp16, bf16}: MultimodalClassifier from the oracle's parameters, one autograd step with CrossEntropyLoss in train mode
(the fused and the graphed step are held bit-identical to it, tests/test_model_gpu.py), and the four bars: per parameter, per row, the
exact zeros, the pooled features of model.encode.  Every measurement goes through conftest.parity_log (profiles/r32_step_rows.txt is one
run's output).  The bars, the cases and what they catch are checked on the CPU in tests/test_step_rows.py.
"""
import math

import pytest
import torch

import step_restatement as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
LR = 2e-5


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import multimodal_propaganda_meme_classification_amd as m
    return m


def _make(pkg, name, dt):
    c = R.case(name)
    d = c.cfg.to_dict()
    d["compute_dtype"] = dt
    model = pkg.MultimodalClassifier.from_config(pkg.ModelConfig.from_dict(d), init=False)
    model.load_state_dict(R.params(c, F32))
    return model.to("cuda").train(), c


def _autograd_step(pkg, model, c):
    dev = [t.cuda() for t in (c.text, c.image, c.mask, c.labels)]
    crit = pkg.CrossEntropyLoss()
    model.zero_grad()
    out = model(dev[0], dev[1], dev[2])
    loss = crit(out, dev[3])
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), loss.detach()


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("name", list(R.CASES))
def test_every_gradient_row_within_the_derived_bars(pkg, name, dt):
    from conftest import parity_log
    model, c = _make(pkg, name, dt)
    assert model.config.stream_scale == R.stream_scale(R.DTYPES[dt])
    b = R.bars(name, R.DTYPES[dt])
    with torch.no_grad():
        tf, vf = model.encode(c.text.cuda(), c.image.cuda(), c.mask.cuda())
        tf, vf = tf.float().cpu(), vf.float().cpu()
    _autograd_step(pkg, model, c)
    got = {k: p.grad.detach().float().cpu() for k, p in model.named_parameters()}
    assert set(got) == set(b.g64)
    tag = f"[step rows {name} {dt}]"
    rep = R.check(b, got, tf, vf, tag=tag)
    for line in rep.lines:
        parity_log(line)
    share, live = b.visible_share()
    k, i, r = rep.worst_row
    parity_log(f"{tag} summary: worst parameter ratio {rep.worst_param[1]:.2f} ({rep.worst_param[0]}); worst row ratio {r:.2f} ({k} row {i}); "
               f"{rep.rows_compared} of {rep.rows_total} rows compared against a bar (the others exactly zero), {share:.3f} of them at "
               f">= 2 bars; bars = {R.FACTOR:g} x emulation; violations {len(rep.violations)}")
    assert not rep.violations, "\n".join([tag] + rep.violations)


def _adam64(p, g, lr, b1, b2, eps, clip):
    """torch.optim.Adam's first step (m = v = 0, no weight decay) in float64, with clip_grad_norm_'s coefficient in front."""
    coef = 1.0
    if clip is not None:
        coef = min(1.0, clip / (float(g.norm()) + 1e-6))
    gg = g * coef
    m, v = (1.0 - b1) * gg, (1.0 - b2) * gg * gg
    upd = (lr / (1.0 - b1)) * (m / (v.sqrt() / math.sqrt(1.0 - b2) + eps))
    return p - upd, upd, coef


@pytest.mark.parametrize("clip", [None, 1.0], ids=["plain", "clip1"])
@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_adam_step_on_the_devices_own_gradients(pkg, dt, clip):
    """One memehip.Adam step (csrc/optim.hip: adam_kernel, adam_rows_kernel) applied to the gradients the device itself computed, against
    float64 Adam applied to those same gradients, element by element over the whole flat buffer.

    The bound, from the operations of adam_update4 at the first step (m = v = 0, weight decay 0; u = 2^-24, one f32 rounding):
      p' = p - U,  U = step * (mm / (sqrtf(v2) * isb + eps))
      gg    = g * gs                      plain: gs = 1, exact.  clipped: gs carries the clip coefficient's error c (below)
      mm    = (1 - b1) * gg               u, and 1 - fl(b1) for 1 - b1 (the f32 hyper-parameter): d1 = u b1 / (1 - b1)
      v2    = (1 - b2) * gg * gg          2 u, and d2 = u b2 / (1 - b2); the square root halves both: u + d2 / 2
      sqrtf, the division                 4 u each (2 ulp: covers a build without correctly rounded sqrt / divide)
      * isb, + eps                        isb as f32 u, the product u, the sum u (eps's own rounding is smaller than the sum's)
      step  = lr * inv_bc1                lr as f32 u, inv_bc1 as f32 u, the product u
      step * quotient                     u
    so |U - U64| <= E |U64| with E = d1 + d2 / 2 + 17 u (+ c), times (1 + E) for the second order, and the new parameter carries one
    more rounding, u |p'| (a fused multiply-subtract only removes one).  U's sensitivity to a relative change of g is
    eps' / (|g| + eps') <= 1, so the clip coefficient's error enters at most once: c = D u / 2 + 5 u, D the longest chain of f32
    additions and multiplications behind a term of mh_sumsq_f32's sum of squares (per thread 8 per 4-element vector, 6 + 4 for the
    wave and workgroup sums, the same for the final kernel), halved by the square root; then sqrtf, * |gs|, + 1e-6, the division and
    the product with gs, u each.
    Rows of the word table that never had a gradient are skipped by adam_rows_kernel: float64 Adam with g = 0 leaves them alone too.
    Wherever the engine keeps a 16-bit shadow of a weight (the first layout.n_shadow elements), the shadow is the round-to-nearest-even
    of the new f32 parameter, bit for bit."""
    from conftest import parity_log
    name = "tiny_cls"
    model, c = _make(pkg, name, dt)
    _autograd_step(pkg, model, c)
    P0, G = model.flat_params.clone(), model.flat_grads.clone()
    b1, b2, eps = 0.9, 0.999, 1e-8
    opt = pkg.Adam(model.parameters(), lr=LR, betas=(b1, b2), eps=eps, max_grad_norm=clip)
    opt.step()
    torch.cuda.synchronize()
    assert opt.skipped_steps == 0
    assert torch.equal(model.flat_grads, G), "the optimizer step changed the gradients"
    P1, SH = model.flat_params.detach().cpu(), model.flat_shadow.detach().cpu()
    p64, g64 = P0.cpu().to(F64), G.cpu().to(F64)
    ref, upd, coef = _adam64(p64, g64, LR, b1, b2, eps, clip)
    u = 2.0 ** -24
    E = u * b1 / (1.0 - b1) + 0.5 * u * b2 / (1.0 - b2) + 17 * u
    if clip is not None:
        n4 = G.numel() // 4
        nb = min(1024, max(1, (G.numel() // 32 + 1 + 255) // 256))
        D = 8 * math.ceil(n4 / (nb * 256)) + 10 + math.ceil(nb / 256) + 10
        E += 0.5 * D * u + 5 * u
    bound = E * (1.0 + E) * upd.abs() + u * torch.maximum(ref.abs(), p64.abs())
    err = (P1.to(F64) - ref).abs()
    moved = int((P1 != P0.cpu()).sum())
    worst = float((err / bound.clamp_min(1e-300)).max())
    parity_log(f"[step rows {name} {dt}] Adam {'clip 1.0' if clip else 'plain'}: clip coefficient {coef:.4f}, {moved} of {P1.numel()} elements moved, "
               f"max |p - p64| {float(err.max()):.3e} (lr {LR:g}), worst error / bound {worst:.3f} (E = {E:.2e})")
    assert moved > P1.numel() // 2
    over = err > bound
    assert not bool(over.any()), (int(over.sum()), int(over.nonzero()[0]), worst)
    # untouched word rows stay as they were, bit for bit
    spec = model.layout.spec[R.WORD]
    rows = P1[spec.offset:spec.offset + spec.numel].view(spec.shape)
    unused = torch.ones(spec.shape[0], dtype=torch.bool)
    unused[c.text.unique()] = False
    unused[c.cfg.text.pad_token_id] = True
    assert torch.equal(rows[unused], P0.cpu()[spec.offset:spec.offset + spec.numel].view(spec.shape)[unused])
    # the 16-bit shadow of every GEMM weight
    ns = model.layout.n_shadow
    assert SH.numel() == ns and SH.dtype == R.DTYPES[dt]
    want = P1[:ns].to(R.DTYPES[dt])
    same = SH.view(torch.int16) == want.view(torch.int16)
    assert bool(same.all()), f"{int((~same).sum())} of {ns} shadow elements are not the rounding of their f32 parameter"
