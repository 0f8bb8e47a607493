"""The last encoder layer on the pooled rows only (``last_rows="pooled"``, the default) against every row (``"all"``), MI355X only.

The head reads one row per sample and tower; behind the last attention core every block is row-wise, so ``"pooled"`` gathers those
B rows (``mh_rows_gather``), runs out-proj / LayerNorm / FFN forward and backward on ``[B, D]`` panels and scatters the out-proj
input gradient back with zero fill (``mh_rows_scatter_zero``).  What must hold, and is asserted here at the ``bench.py --tiny``
widths (hidden 128, 2 layers, 2 heads, image 32) in both storage types:

* forward bit-identical: loss, correct count, logits, pooled features, and every saved activation of the last layer at the
  pooled rows (a GEMM output row depends on its own A row only, a LayerNorm row on itself);
* bit-identical gradients for everything that does not contract over the compacted rows: layers 0..L-2, embeddings, head, the
  QKV weights / biases of layer L-1, and the dgrad panels at the rows both forms have (df, dh, da / dh, dxp: the buffers the
  2-layer model does not overwrite later in the step);
* the weight / bias gradients of out-proj, FFN up, FFN down and the LayerNorm gamma / beta of layer L-1 and the final ViT
  LayerNorm contract over rows: both forms are f32 sums of the same <= B non-zero products per element (16-bit x 16-bit
  products are exact in f32), in another order.  Any order is within (B - 1) 2^-24 sum|terms| of the exact sum, so the two are
  within ``2 B 2^-24 sum_b |dy_b| |x_b|`` of each other, element by element; that bound is asserted, not a tuned number;
* parameters after Adam: equal where the gradient is bit-identical.  Elsewhere the first Adam step is
  ``lr g / (|g| + eps)`` (zero moments), Lipschitz in g with constant lr / eps and never larger than lr, so the two parameters
  differ by at most ``lr min(2, bound / eps)`` plus one rounding of the parameter each (2 * 2^-24 |p|).

Two steps on different batches.  After step 1 is compared, the ``"pooled"`` model takes over the ``"all"`` model's parameters,
shadow and moments (they may differ in the last bit where the bound applies), so that step 2 -- stale buffers, the scatter in the
place of the zero fill, another live-row count -- can be compared bit for bit again.
"""
import os
import subprocess
import sys

import pytest
import torch
from conftest import parity_log

pytestmark = pytest.mark.gpu

LR, EPS = 2e-5, 1e-8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_ENV = "MEMEHIP_LAST_ROWS_TEST_CHILD"
DTYPES = ("fp16", "bf16")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import multimodal_propaganda_meme_classification_amd as m
    return m


def _oracle():
    from oracle import meme_oracle as O
    return O


_PARAMS = {}


def _params(O, cfg):
    key = repr(cfg)
    if key not in _PARAMS:
        _PARAMS[key] = O.init_params(cfg, 29)
    return _PARAMS[key]


def _model(pkg, O, cfg, dtype, pack, dropout=False):
    mc = pkg.ModelConfig.from_dict(cfg.to_dict())
    mc.compute_dtype, mc.pack_text = dtype, pack
    if dropout:
        mc.with_reference_dropout()
    model = pkg.MultimodalClassifier.from_config(mc, init=False)
    model.load_state_dict(_params(O, cfg))
    model.to("cuda").train()
    model.manual_seed(77)
    return model


def _batches(O, cfg, B, S, lens_first):
    """Two batches with different masks; the first one's sequence lengths are `lens_first` (None: the oracle's ragged ones)."""
    out = []
    for k, seed in enumerate((201, 202)):
        text, image, mask, labels = O.synthetic_batch(cfg, B, S, seed=seed)
        if k == 0 and lens_first is not None:
            lens = torch.tensor(lens_first)
            mask = (torch.arange(S)[None] < lens[:, None]).to(torch.int64)
            text = text.clamp(min=5) * mask
        out.append([t.cuda() for t in (text, image, mask, labels)])
    return out


class _Side:
    def __init__(self, pkg, O, cfg, dtype, pack, B, S, last_rows, **kw):
        self.model = _model(pkg, O, cfg, dtype, pack)
        self.opt = pkg.Adam(self.model.parameters(), lr=LR, eps=EPS, model=self.model)
        self.step = pkg.GraphedStep(self.model, self.opt, B, S, last_rows=last_rows, **kw)
        self.plan = self.step.plan
        assert self.plan.last_rows == last_rows and self.plan.packed == pack
        self.loss = None

    def run(self, batch):
        self.step.load_batch(*batch)
        self.loss, _ = self.step.step()

    def state(self):
        return dict(flat_params=self.model.flat_params, flat_shadow=self.model.flat_shadow, adam_m=self.opt._flat["M"],
                    adam_v=self.opt._flat["V"])

    def outputs(self):
        b = self.plan.buf
        return dict(loss=self.loss, ncorrect=b["ncorrect"], logits=b["logits"], pooled=b["h.pooled"], flat_grads=self.model.flat_grads)

    def close(self):
        self.step.close()
        self.step = self.model = self.opt = self.plan = None


def _rows_of(plan, cfg, B, S):
    """(text rows, image rows) of the pooled positions in a plan's full row buffers"""
    if plan.packed:
        t_rows = plan.buf["pk.pool_rows"].long()
    else:
        t_rows = torch.arange(B, device="cuda") * S + (0 if cfg.pool == "cls" else S - 1)
    nt = (cfg.image.image_size // cfg.image.patch) ** 2 + 1
    return t_rows, torch.arange(B, device="cuda") * nt


def _row_sum_specs(cfg):
    """name -> how the parameter's gradient contracts over the compacted rows: ("w", dy buffer, x buffer) for a weight,
    ("b", dy buffer) for a bias / LayerNorm beta, ("g", dy buffer, x buffer, mean, rstd) for a LayerNorm gamma.  Buffer names are
    the "pooled" plan's."""
    lt, li = cfg.text.layers - 1, cfg.image.layers - 1
    T, I = f"bert.encoder.layer.{lt}.", f"image_model.encoder.layer.{li}."
    sp = {}

    def lin(name, dy, x):
        sp[name + ".weight"], sp[name + ".bias"] = ("w", dy, x), ("b", dy)

    def ln(name, dy, x, m, r):
        sp[name + ".weight"], sp[name + ".bias"] = ("g", dy, x, m, r), ("b", dy)

    lin(T + "output.dense", "t.dfrows", f"t{lt}.g")
    lin(T + "intermediate.dense", "t.dhrows", f"t{lt}.y")
    lin(T + "attention.output.dense", "t.darows", f"t{lt}.pctx")
    ln(T + "output.LayerNorm", "t.dXrows", f"t{lt}.f", f"t{lt}.m2", f"t{lt}.r2")
    ln(T + "attention.output.LayerNorm", "t.dyrows", f"t{lt}.a", f"t{lt}.m1", f"t{lt}.r1")
    lin(I + "output.dense", "i.dXrows", f"i{li}.g")
    lin(I + "intermediate.dense", "i.dhrows", f"i{li}.w")
    lin(I + "attention.output.dense", "i.dxprows", f"i{li}.pctx")
    ln(I + "layernorm_after", "i.dwrows", f"i{li}.xp", f"i{li}.m2", f"i{li}.r2")
    ln("image_model.layernorm", "i.dXf", f"i.x{li + 1}", "i.mf", "i.rf")
    return sp


def _grad_bounds(side, cfg, B):
    """name -> 2 B 2^-24 sum_b |dy_b| |x_b| per element (module docstring), from the "pooled" plan's own panels"""
    buf, gs = side.plan.buf, float(side.model.config.stream_scale)
    out = {}
    for name, spec in _row_sum_specs(cfg).items():
        dy = buf[spec[1]].float().abs() / gs
        if spec[0] == "w":
            s = dy.t() @ buf[spec[2]].float().abs()
        elif spec[0] == "b":
            s = dy.sum(0)
        else:
            xh = (buf[spec[2]].float() - buf[spec[3]][:, None]) * buf[spec[4]][:, None]
            s = (dy * xh.abs()).sum(0)
        out[name] = 2.0 * B * 2.0 ** -24 * s.double()
    return out


def _compare_step(pooled, full, cfg, B, S, step, tag):
    layout = pooled.model.layout
    po, fo = pooled.outputs(), full.outputs()
    for key in ("loss", "ncorrect", "logits", "pooled"):
        assert torch.equal(po[key], fo[key]), f"[{tag}] step {step}: {key} differs between 'pooled' and 'all'"
    # saved activations and dgrad panels of the last layers, at the rows both forms have
    t_rows, i_rows = _rows_of(full.plan, cfg, B, S)
    lt, li = cfg.text.layers - 1, cfg.image.layers - 1
    pb, fb = pooled.plan.buf, full.plan.buf
    pairs = [(f"t{lt}.{k}", f"t{lt}.{k}", t_rows) for k in ("a", "y", "h", "g", "f", "m1", "r1", "m2", "r2")]
    pairs += [(f"t{lt}.pctx", f"t{lt}.ctx", t_rows), (f"t.x{lt + 1}", f"t.x{lt + 1}", t_rows), ("t.xlast32", "t.xlast32", t_rows)]
    pairs += [(f"i{li}.{k}", f"i{li}.{k}", i_rows) for k in ("xp", "w", "h", "g", "m2", "r2")]
    pairs += [(f"i{li}.pctx", f"i{li}.ctx", i_rows), (f"i.x{li + 1}", f"i.x{li + 1}", i_rows), ("i.xf32", "i.xf32", i_rows),
              ("i.mf", "i.mf", i_rows), ("i.rf", "i.rf", i_rows)]
    pairs += [("t.dXrows", "t.dX0", t_rows), ("t.dfrows", f"t.df{lt % 3}", t_rows), ("t.dhrows", f"t.dh{lt & 1}", t_rows),
              ("t.darows", f"t.da{lt & 1}", t_rows), ("i.dXf", "i.dXf", i_rows), ("i.dXrows", "i.dX0", i_rows),
              ("i.dhrows", f"i.dh{li & 1}", i_rows), ("i.dxprows", f"i.dxp{li & 1}", i_rows)]
    for pn, fn, rows in pairs:
        assert torch.equal(pb[pn], fb[fn][rows]), f"[{tag}] step {step}: {pn} != rows of {fn}"
    # the scattered full buffers of the "pooled" form: the panel at the pooled rows, zero elsewhere (live rows only)
    for pn, fn, rows, n in (("t.darows", f"t.da{lt & 1}", t_rows, int(pb["pk.n_rows"]) if pooled.plan.packed else B * S),
                            ("i.dxprows", f"i.dxp{li & 1}", i_rows, fb[f"i.dxp{li & 1}"].shape[0])):
        want = torch.zeros_like(pb[fn][:n])
        want[rows] = pb[pn]
        assert torch.equal(pb[fn][:n], want), f"[{tag}] step {step}: scattered {fn}"
    # gradients and the parameters after Adam, parameter by parameter
    bounds = _grad_bounds(pooled, cfg, B)
    pg, fg = po["flat_grads"], fo["flat_grads"]
    pp, fp = pooled.model.flat_params, full.model.flat_params
    worst, n_exact, seen = {}, 0, set()
    for sp in layout.specs:
        sl = slice(sp.offset, sp.offset + sp.numel)
        if sp.name not in bounds:
            assert torch.equal(pg[sl], fg[sl]), f"[{tag}] step {step}: gradient of {sp.name} must be bit-identical"
            assert torch.equal(pp[sl], fp[sl]), f"[{tag}] step {step}: parameter {sp.name} after Adam must be bit-identical"
            n_exact += sp.numel
            continue
        seen.add(sp.name)
        bd = bounds[sp.name].reshape(-1)
        assert bd.numel() == sp.numel, sp.name
        diff = (pg[sl].double() - fg[sl].double()).abs()
        ratio = float((diff / bd.clamp(min=1e-300)).max()) if float(diff.max()) > 0 else 0.0
        worst[sp.name] = (float(diff.max()), ratio)
        parity_log(f"[{tag}] step {step} {sp.name}: max |dg| {float(diff.max()):.3e}, max |dg| / bound {ratio:.3e}")
        assert bool((diff <= bd).all()), f"[{tag}] step {step}: gradient of {sp.name} leaves 2 B 2^-24 sum|dy||x| (ratio {ratio:.3f})"
        if step == 0:      # first Adam step from zero moments
            pbound = LR * torch.minimum(torch.full_like(bd, 2.0), bd / EPS) + 2.0 * 2.0 ** -24 * fp[sl].double().abs()
            pd = (pp[sl].double() - fp[sl].double()).abs()
            assert bool((pd <= pbound).all()), f"[{tag}] parameter {sp.name} after Adam: {float(pd.max()):.3e} beyond lr min(2, bound / eps)"
    assert seen == set(bounds), sorted(set(bounds) - seen)
    return n_exact, worst


def _pair(pkg, tag, dtype, pool, pack, B, S, lens_first, **kw):
    O = _oracle()
    cfg = O.tiny_config(pool)
    pooled = full = None
    try:
        pooled = _Side(pkg, O, cfg, dtype, pack, B, S, "pooled", **kw)
        full = _Side(pkg, O, cfg, dtype, pack, B, S, "all", **kw)
        assert len(pooled.plan.fwd) == len(full.plan.fwd) + 1, "one gather launch more"
        for step, batch in enumerate(_batches(O, cfg, B, S, lens_first)):
            if step:       # same starting point for the second step (module docstring)
                for a, b in zip(pooled.state().values(), full.state().values()):
                    a.copy_(b)
            pooled.run(batch)
            full.run(batch)
            torch.cuda.synchronize()
            n_exact, worst = _compare_step(pooled, full, cfg, B, S, step, tag)
            w = max(worst.values(), key=lambda x: x[1])
            parity_log(f"[{tag}] step {step}: {n_exact} gradient elements bit-identical; row-sum gradients: worst |dg| / bound {w[1]:.3e}")
    finally:
        for s in (pooled, full):
            if s is not None:
                s.close()
        torch.cuda.empty_cache()


EAGER = dict(use_graph=False, overlap_wgrad=False, overlap_optimizer=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cls_packed_ragged(pkg, dtype):
    """B = 3, S = 16, pool "cls", packed text; one sequence of a single token, one of full length."""
    _pair(pkg, f"last-rows cls packed {dtype}", dtype, "cls", True, 3, 16, [1, 16, 7], **EAGER)


@pytest.mark.parametrize("dtype", DTYPES)
def test_last_dense_pooled_row_is_padding(pkg, dtype):
    """pool "last" on a dense text tower: the pooled row is S - 1, in the last block, and padding for the short sequences."""
    _pair(pkg, f"last-rows last dense {dtype}", dtype, "last", False, 3, 16, [1, 16, 7], **EAGER)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,pool,pack", [(1, 16, "cls", True), (33, 40, "last", True), (33, 40, "last", False)])
def test_one_sample_and_more_than_one_panel(pkg, dtype, B, S, pool, pack):
    """B = 1; and B = 33, S = 40: 165 image rows (two 128-row panels) against a 33-row compact panel, the text pooled row in the
    second 32-row attention block."""
    _pair(pkg, f"last-rows B{B} S{S} {pool} {'packed' if pack else 'dense'} {dtype}", dtype, pool, pack, B, S, None, **EAGER)


# ---- the schedule does not change what the pooled form computes ----------------------------------------------------------------------------

SCHEDULES = (("eager two-stream", dict(use_graph=False)), ("graph, no overlap", dict(use_graph=True, overlap_wgrad=False, overlap_optimizer=False)),
             ("graph, wgrad overlap only", dict(use_graph=True, overlap_optimizer=False)),
             ("graph, optimizer overlap only", dict(use_graph=True, overlap_wgrad=False)), ("graph, both", dict(use_graph=True)))


def test_pooled_form_is_the_same_under_every_schedule(pkg, request):
    """Eager and graphed, both overlap switches off and on: bitwise equal to the one-stream sequential step after each of three
    steps, as tests/test_step_schedules_gpu.py asserts for the full form.  Always in a fresh child process: multi-stream hipGraph
    capture depends on what the process has done before (streams handed out by torch's pool, RCCL communicators created or
    destroyed: profiles/r04_segfault_record.md), and this file must neither inherit such history nor leave any to the files that
    run after it in the same pytest process."""
    if os.environ.get(CHILD_ENV) != "1":
        env = dict(os.environ)
        env[CHILD_ENV] = "1"
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", f"{request.node.path}::{request.node.name}", "-q", "-x",
                                                                                "-p", "no:cacheprovider"]
        out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and " passed" in out.stdout, out.stdout[-4000:] + out.stderr[-2000:]
        return
    for dtype in DTYPES:
        _schedules_equal(pkg, dtype)


def _schedules_equal(pkg, dtype):
    O = _oracle()
    cfg = O.tiny_config("last")
    B, S = 5, 40
    sides = []
    try:
        sides.append(_Side(pkg, O, cfg, dtype, True, B, S, "pooled", **EAGER))
        for _, kw in SCHEDULES:
            sides.append(_Side(pkg, O, cfg, dtype, True, B, S, "pooled", **kw))
            if kw["use_graph"]:
                assert sides[-1].step.use_graph
        batches = _batches(O, cfg, B, S, [1, 40, 33, 9, 32])
        n = 0
        for step, bi in enumerate((0, 1, 0)):
            for s in sides:
                s.run(batches[bi])
            torch.cuda.synchronize()
            ref = dict(sides[0].state(), **sides[0].outputs())
            for (name, kw), s in zip(SCHEDULES, sides[1:]):
                if kw["use_graph"]:
                    assert s.step.graphs is not None, f"'{name}' did not replay a hipGraph"
                for key, a in dict(s.state(), **s.outputs()).items():
                    assert torch.equal(a, ref[key]), f"pooled form, schedule '{name}', step {step}: {key} differs from the sequential step"
                    n += a.numel()
        parity_log(f"[last-rows schedules {dtype}] 3 steps x {len(SCHEDULES)} schedules == sequential: {n} elements bit for bit")
    finally:
        for s in sides:
            s.close()
        torch.cuda.empty_cache()


# ---- fall-backs ----------------------------------------------------------------------------------------------------------------------------

def test_plans_that_need_every_row_fall_back(pkg):
    O = _oracle()
    cfg = O.tiny_config("cls")
    model = _model(pkg, O, cfg, "fp16", True)
    eng = model._get_engine()
    assert eng.plan(3, 16, True).last_rows == "pooled" and eng.plan(3, 16, True, features=True).last_rows == "pooled"
    assert eng.plan(3, 16, True, last_rows="all").last_rows == "all"
    seq = eng.plan(3, 16, True, features="sequence")
    assert seq.last_rows == "all" and tuple(seq.buf["t.xlast32"].shape) == (3 * 16, cfg.text.hidden)
    with pytest.raises(ValueError):
        eng.plan(3, 16, True, last_rows="some")
    # dropout masks are indexed by the full row: such plans keep every row
    drop = _model(pkg, O, cfg, "fp16", True, dropout=True)
    opt = pkg.Adam(drop.parameters(), lr=LR, model=drop)
    gs = pkg.GraphedStep(drop, opt, 3, 16, **EAGER)
    assert gs.plan.dropout_on and gs.plan.last_rows == "all"
    gs.close()
    assert drop.eval()._get_engine().plan(3, 16, False).last_rows == "pooled"        # eval: no dropout, pooled rows again
    # a pooling over all positions reads the whole last hidden state: its plan keeps it complete
    tc = pkg.TextConfig(vocab_size=512, hidden=128, layers=2, heads=2, intermediate=256, max_position=64, type_vocab=2)
    clf = pkg.TextClassifier(tc, pooling_type="mean", num_classes=2, compute_dtype="fp16").cuda()
    clf.train()
    text, _, mask, labels = (t.cuda() for t in O.synthetic_batch(cfg, 3, 16, seed=5))
    loss, logits = clf(input_ids=text, attention_mask=mask, labels=labels)
    loss.backward()
    plans = list(clf.model.inner._get_engine().plans.values())
    assert plans and all(p.features == "sequence" and p.last_rows == "all" for p in plans)
    assert bool(torch.isfinite(logits).all())


# ---- the two kernels -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16))
@pytest.mark.parametrize("D", (64, 768))
@pytest.mark.parametrize("n_jobs", (1, 5))
def test_rows_gather_and_scatter_zero_kernels(pkg, dtype, D, n_jobs):
    """mh_rows_gather / mh_rows_scatter_zero against index_select / index_copy_ into zeros, bitwise: index arrays (one holding the
    last row, one holding row 0 and adjacent rows) and arithmetic rows, several jobs per launch, rows_dev smaller than the buffer
    (rows past it keep their sentinel)."""
    from multimodal_propaganda_meme_classification_amd import ops
    g = torch.Generator(device="cpu").manual_seed(1000 + D + n_jobs)
    I32 = torch.int32
    shapes = [(197, [0, 1, 2, 57, 196], None), (300, None, (6, 50, 3)), (41, [40], None), (64, None, (64, 1, 0)), (130, [5, 6, 128, 129], None)][:n_jobs]
    gather, scatter, checks = [], [], []
    for k, (rows, idx, arith) in enumerate(shapes):
        if idx is None:
            n, stride, off = arith
            idx_l = [b * stride + off for b in range(n)]
            names = dict(stride=stride, offset=off)
        else:
            idx_l, n = idx, len(idx)
            names = dict(idx=torch.tensor(idx, dtype=I32).cuda())
        it = torch.tensor(idx_l).cuda()
        full = torch.randn((rows, D), generator=g).to(dtype).cuda()
        out = torch.full((n, D), 7.0, dtype=dtype).cuda()
        gather.append(dict(names, src=full, dst=out))
        checks.append((out, full.index_select(0, it), f"gather job {k}"))
        # scatter: live rows = all of them (even jobs) or a count that cuts the last indexed rows off (odd jobs)
        live = rows if k % 2 == 0 else max(1, idx_l[-1])
        comp = torch.randn((n, D), generator=g).to(dtype).cuda()
        dst = torch.full((rows, D), -3.0, dtype=dtype).cuda()
        want = torch.full((rows, D), -3.0, dtype=dtype).cuda()
        want[:live] = 0
        keep = it < live
        want.index_copy_(0, it[keep], comp[keep])
        scatter.append(dict(names, src=comp, dst=dst, rows_dev=None if live == rows else torch.tensor([live], dtype=I32).cuda()))
        checks.append((dst, want, f"scatter job {k} (live rows {live} of {rows})"))
    ops.rows_gather(gather)
    ops.rows_scatter_zero(scatter)
    torch.cuda.synchronize()
    for got, want, what in checks:
        assert torch.equal(got, want), what
    # an index outside the buffer is refused (arithmetic rows) -- the kernels never leave their buffers
    with pytest.raises(pkg._lib.MemehipError):
        ops.rows_gather([dict(stride=10, offset=5, src=torch.zeros((20, D), dtype=dtype).cuda(), dst=torch.zeros((3, D), dtype=dtype).cuda())])


def test_rows_job_struct_matches_the_header(pkg, tmp_path):
    import ctypes
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "memehip.h"\nint main(void){printf("%zu\\n", sizeof(MhRowsJob));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout) == ctypes.sizeof(pkg._lib.MhRowsJob) == 56
