"""The fine-tune step's gradients, row by row, against float64 (not a test module; no GPU code).

``CASES``      the smallest batches at which the joins between the kernels -- launch plan, padding-free row counts, LayerNorm partials,
               embedding scatter, pooled-row last layer -- can still go wrong (``case`` builds one from its seed).
``run``        one step of the oracle (oracle/meme_oracle.py) on a case: logits, loss, every parameter gradient and the two pooled
               tower features, in ``dtype`` arithmetic with the engine's 16-bit ``storage`` points or without (cached; read-only).
``grads``      its gradients.  g64 = grads(c, float64, None); gemu = grads(c, float32, fp16 | bf16), the EMULATION: float32 arithmetic
               with every value the engine keeps in 16 bits rounded where the engine rounds it (the points are listed, each with its
               buffer, in the comments of text_tower / image_tower / _mha there).
``Bars``       what a device gradient g is held to, all from g64 and gemu alone:
                 per parameter   ||g - g64||_F <= FACTOR ||gemu - g64||_F          (.key.bias, analytically zero: < 1e-4)
                 per row         a row = a slice along dim 0 of a parameter with >= 2 dimensions; rho = ||gemu - g64||_F / ||g64||_F
                                 of its parameter, n its row count:
                                 ||g_r - g64_r|| <= FACTOR max(||gemu_r - g64_r||, rho ||g64_r||, rho ||g64||_F / sqrt(n))
                                 (the 2nd and 3rd term: a row is not judged against an emulation error that happens to be near 0)
                 exact zeros     a row that is exactly zero in float64 (word rows of ids not in the batch, the PAD row, position
                                 rows at or beyond S, token-type row 1) is exactly zero
                 pooled          RMS error of the pooled text / image features <= FACTOR x the emulation's RMS error
               FACTOR = 4 is the one the conv towers use (tests/test_resnet_gpu.py, test_convnext_train_gpu.py): room for another
               summation order, not for a wrong term.
``check``      applies the bars to a set of gradients and returns every measurement and every violation.
``row_terms``  the per-token-row terms of a LayerNorm's dgamma or of a Linear's weight gradient (what the engine sums over rows), for
               the fault injections of tests/test_step_rows.py.
"""
import contextlib
import functools
import math
from collections import namedtuple

import torch

from oracle import meme_oracle as O

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
FACTOR = 4.0
DTYPES = {"fp16": F16, "bf16": BF16}
WORD = "bert.embeddings.word_embeddings.weight"

Case = namedtuple("Case", "name cfg seed text image mask labels lens")
Step = namedtuple("Step", "logits loss grads text_feat image_feat")

# name -> (pool, B, S, image size, clip-style switches, parameter seed, batch seed, sequence lengths).  Every set of lengths holds a
# full-length row and a row of length 1; two_tiles has 181 live text rows (a prime: one full 128-row tile and a partial one).
CASES = {
    "tiny_cls": ("cls", 5, 24, 32, False, 21, 31, (24, 1, 13, 7, 18)),
    "tiny_last": ("last", 5, 24, 32, False, 22, 32, (9, 24, 1, 20, 15)),
    "two_tiles": ("cls", 7, 40, 64, False, 23, 33, (40, 1, 33, 17, 29, 38, 23)),
    "clip_style": ("cls", 5, 24, 32, True, 24, 34, (1, 17, 24, 11, 5)),
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    pool, B, S, size, clip, seed, bseed, lens = CASES[name]
    cfg = O.tiny_config(pool)
    cfg.image.image_size = size
    if clip:        # config 5's switches (oracle.config5): CLIP vision tower, DistilBERT-style text tower
        cfg.image.pre_ln, cfg.image.act, cfg.image.patch_bias, cfg.image.ln_eps = True, "quick_gelu", False, 1e-5
        cfg.text.type_vocab = 0
    _, image, _, labels = O.synthetic_batch(cfg, B, S, seed=bseed)
    # (synthetic_batch pads by lengths of its own: the ids are drawn here, for the lengths of the case)
    text = torch.randint(5, cfg.text.vocab_size, (B, S), generator=torch.Generator().manual_seed(bseed), dtype=torch.int64)
    lens = torch.tensor(lens)
    assert lens.numel() == B and int(lens.max()) == S and int(lens.min()) == 1
    mask = (torch.arange(S)[None] < lens[:, None]).to(torch.int64)
    full, other = int(lens.argmax()), int(lens.argsort()[-2])
    text[full, 9] = text[full, 5]            # an id twice in one row ...
    text[other, 3] = text[full, 5]           # ... and in a second row (three occurrences in the batch)
    text[full, 7] = text[full, 11] = 4       # an id exactly twice in the batch, in one row (synthetic_batch draws ids >= 5)
    text = text * mask                       # PAD id 0 on the padded positions
    text[:, 0] = 2                           # the [CLS]-like id: once in every row
    labels[0], labels[1] = 0, 1              # both classes present
    assert cfg.text.pad_token_id == 0 and int((text == 0).sum()) > 0
    return Case(name, cfg, seed, text, image, mask, labels, lens)


def params(c: Case, dtype=F32):
    return {k: v.to(dtype) for k, v in O.init_params(c.cfg, c.seed).items()}


def _step(c: Case, p, dtype, storage, text=None) -> Step:
    cfg = c.cfg
    text = c.text if text is None else text
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    st = O.Storage(storage)
    tf = O.pool_text(O.text_tower(leaves, text, c.mask, cfg.text, storage=st), cfg.pool)
    vf = O.image_tower(leaves, c.image.to(dtype), cfg.image, storage=st)[:, 0]
    lin = torch.nn.functional.linear
    t = lin(tf, leaves["bert_fc.weight"], leaves["bert_fc.bias"])
    v = lin(vf, leaves["image_fc.weight"], leaves["image_fc.bias"])
    f = lin(torch.cat((t, v), dim=1), leaves["fusion_fc.weight"], leaves["fusion_fc.bias"])
    logits = lin(f, leaves["output_fc.weight"], leaves["output_fc.bias"])
    loss = O.cross_entropy(logits, c.labels)
    loss.backward()
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return Step(logits.detach(), loss.detach(), g, tf.detach(), vf.detach()), leaves


@functools.lru_cache(maxsize=None)
def run(name: str, dtype=F64, storage=None) -> Step:
    c = case(name)
    return _step(c, params(c, dtype), dtype, storage)[0]


def grads(name: str, dtype=F64, storage=None):
    return run(name, dtype, storage).grads


def stream_scale(storage) -> float:
    """ModelConfig.stream_scale: the power of two the 16-bit gradient stream carries."""
    return O.Storage(storage).scale


# ---- the per-row terms of a sum over token rows ------------------------------------------------------------------------

@contextlib.contextmanager
def _tap(leaves, name, out):
    """Records, for the LayerNorm or Linear whose weight is the leaf ``name``, the input and the gradient at the output."""
    fn = torch.nn.functional
    real_ln, real_lin = fn.layer_norm, fn.linear

    def hook(y, x, kind):
        out["x"], out["kind"] = x.detach(), kind
        y.register_hook(lambda g: out.__setitem__("dy", g.detach()))

    def ln(x, shape, weight=None, bias=None, eps=1e-5):
        y = real_ln(x, shape, weight, bias, eps)
        if weight is leaves[name]:
            mu, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
            hook(y, (x - mu) * torch.rsqrt(var + eps), "ln")
        return y

    def lin(x, w, b=None):
        y = real_lin(x, w, b)
        src = w
        if w.grad_fn is not None and type(w.grad_fn).__name__.startswith("_RoundSTE"):     # the 16-bit shadow of a leaf
            src = getattr(w.grad_fn.next_functions[0][0], "variable", None)
        if src is leaves[name]:
            hook(y, x, "linear")
        return y

    fn.layer_norm, fn.linear = ln, lin
    try:
        yield
    finally:
        fn.layer_norm, fn.linear = real_ln, real_lin


def row_terms(name: str, param: str, dtype=F32, storage=None):
    """(x [rows, K], dy [rows, N]) of the LayerNorm (x = x-hat, N = K) or Linear whose weight is ``param``: its weight gradient is
    sum_r dy_r (x) x_r (LayerNorm: sum_r dy_r * xhat_r), so the sum without row r is the gradient minus that term."""
    c = case(name)
    out = {}
    p = params(c, dtype)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    with _tap(leaves, param, out):
        st = O.Storage(storage)
        logits = O.forward(leaves, c.text, c.image.to(dtype), c.mask, c.cfg, storage=st)
        O.cross_entropy(logits, c.labels).backward()
    x, dy = out["x"].reshape(-1, out["x"].shape[-1]), out["dy"].reshape(-1, out["dy"].shape[-1])
    full = (dy * x).sum(0) if out["kind"] == "ln" else dy.t() @ x
    ref = leaves[param].grad
    assert float((full - ref).norm()) <= 1e-5 * float(ref.norm()), "the tapped terms do not sum to the gradient"
    return x, dy, out["kind"]


def scattered_once(name: str, dtype, storage, word_id: int):
    """The word-table gradient row of ``word_id`` when only its FIRST occurrence in the batch is scattered: the later occurrences
    read an unused row holding the same values, so the forward pass is the same and the row's gradient is that one term."""
    c = case(name)
    p = params(c, dtype)
    used = set(c.text.flatten().tolist())
    spare = next(i for i in range(c.cfg.text.vocab_size - 1, 0, -1) if i not in used)
    p[WORD][spare] = p[WORD][word_id]
    flat = c.text.flatten().clone()
    where = (flat == word_id).nonzero().flatten()
    assert where.numel() >= 2
    flat[where[1:]] = spare
    step, _ = _step(c, p, dtype, storage, text=flat.view_as(c.text))
    return step.grads[WORD][word_id]


# ---- the bars ----------------------------------------------------------------------------------------------------------

def _rows(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(t.shape[0], -1).to(F64)


class Bars:
    """The bars of one (case, storage dtype), from the float64 gradient and the emulation."""

    def __init__(self, name: str, storage):
        self.name, self.storage = name, storage
        ref, emu = run(name, F64, None), run(name, F32, storage)
        self.ref, self.emu = ref, emu
        self.g64 = {k: v.to(F64) for k, v in ref.grads.items()}
        self.gemu = {k: v.to(F64) for k, v in emu.grads.items()}
        self.param_err = {k: float((self.gemu[k] - v).norm()) for k, v in self.g64.items()}
        self.param_norm = {k: float(v.norm()) for k, v in self.g64.items()}
        self.row_bar, self.row_norm, self.zero_rows = {}, {}, {}
        for k, v in self.g64.items():
            if v.dim() < 2:
                continue
            r64, remu = _rows(v), _rows(self.gemu[k])
            n = r64.shape[0]
            rho = self.param_err[k] / self.param_norm[k]
            nrm = r64.norm(dim=1)
            self.row_norm[k] = nrm
            self.row_bar[k] = FACTOR * torch.maximum(torch.maximum((remu - r64).norm(dim=1), rho * nrm),
                                                     torch.full_like(nrm, rho * self.param_norm[k] / math.sqrt(n)))
            self.zero_rows[k] = (r64 == 0).all(dim=1)
        self.feat_err = {"text": _rms(emu.text_feat, ref.text_feat), "image": _rms(emu.image_feat, ref.image_feat)}

    def param_bar(self, k: str) -> float:
        return FACTOR * self.param_err[k]

    def visible_share(self):
        """Share of the live rows (not exactly zero in float64) whose norm is at least twice their bar: the rows where a lost
        row shows as twice the bar.  -> (share, live rows)."""
        seen = live = 0
        for k, bar in self.row_bar.items():
            lv = ~self.zero_rows[k]
            live += int(lv.sum())
            seen += int((self.row_norm[k][lv] >= 2.0 * bar[lv]).sum())
        return seen / live, live


def _rms(a, b) -> float:
    return float((a.to(F64) - b.to(F64)).pow(2).mean().sqrt())


@functools.lru_cache(maxsize=None)
def bars(name: str, storage) -> Bars:
    return Bars(name, storage)


Report = namedtuple("Report", "lines violations worst_param worst_row rows_compared rows_total")


def check(b: Bars, got, text_feat=None, image_feat=None, tag: str = "") -> Report:
    """Holds the gradients ``got`` (name -> tensor) -- and, when given, the pooled features -- to the bars.  ``lines``: one
    measurement per parameter (device error, emulation error, ratio; for matrices the worst row ratio too); ``violations``: every
    bar that fired, as text."""
    lines, bad = [], []
    worst_p, worst_r = ("", 0.0), ("", -1, 0.0)
    compared = total = 0
    for k, ref in b.g64.items():
        g = got[k].detach().to("cpu", F64)
        err = float((g - ref).norm())
        if ".key.bias" in k:            # analytically zero: the emulation's own error is rounding noise around 0
            lines.append(f"{tag} {k}: hip {err:.3e} (analytically zero, < 1e-4)")
            if not err < 1e-4:
                bad.append(f"{k}: ||g|| = {err:.3e} for an analytically zero gradient")
            continue
        ratio = err / b.param_err[k] if b.param_err[k] > 0 else (0.0 if err == 0 else math.inf)
        line = f"{tag} {k}: hip {err:.3e} emulation {b.param_err[k]:.3e} ratio {ratio:.2f}"
        if ratio > worst_p[1]:
            worst_p = (k, ratio)
        if not err <= b.param_bar(k):
            bad.append(f"{k}: ||g - g64|| = {err:.3e} > {FACTOR:g} x {b.param_err[k]:.3e} (ratio {ratio:.2f})")
        if k in b.row_bar:
            rg, r64 = _rows(g), _rows(ref)
            zero, bar = b.zero_rows[k], b.row_bar[k]
            total += rg.shape[0]
            compared += int((~zero).sum())
            dirty = zero & (rg != 0).any(dim=1)
            if bool(dirty.any()):
                bad.append(f"{k}: rows {dirty.nonzero().flatten().tolist()[:8]} are exactly zero in float64 and are not here")
            rerr = (rg - r64).norm(dim=1)
            rr = torch.where(zero, torch.zeros_like(rerr), rerr / (bar / FACTOR))      # in units of the emulation-side term
            i = int(rr.argmax())
            line += f" worst row {i}: {float(rr[i]):.2f}"
            if float(rr[i]) > worst_r[2]:
                worst_r = (k, i, float(rr[i]))
            over = (~zero) & ~(rerr <= bar)
            if bool(over.any()):
                j = int(torch.where(over, rerr / bar, torch.zeros_like(rerr)).argmax())
                bad.append(f"{k}: {int(over.sum())} row(s) over their bar, worst row {j}: ||g_r - g64_r|| = {float(rerr[j]):.3e} > "
                           f"{float(bar[j]):.3e} (||g64_r|| = {float(b.row_norm[k][j]):.3e})")
        lines.append(line)
    for what, feat, ref in (("text", text_feat, b.ref.text_feat), ("image", image_feat, b.ref.image_feat)):
        if feat is None:
            continue
        err, emu = _rms(feat.detach().cpu(), ref), b.feat_err[what]
        lines.append(f"{tag} pooled {what} features: hip rms {err:.3e} emulation rms {emu:.3e} ratio {err / emu:.2f}")
        if not err <= FACTOR * emu:
            bad.append(f"pooled {what} features: rms error {err:.3e} > {FACTOR:g} x {emu:.3e}")
    return Report(lines, bad, worst_p, worst_r, compared, total)
