"""The benchmarked step's schedules, bit for bit, at the sizes the benchmark runs (MI355X only).

``GraphedStep`` runs the weight-gradient GEMMs of a layer pair on a side stream and the pair's Adam slice behind them, captures
the whole two-stream step into one hipGraph, packs the text tower and keeps the fp16 loss scale on the device.  That is correct
only if the hand-placed cross-stream edges (``Segment.run2``'s fork, ``s.wait("bwd_layer_{l+2}")``, the join in front of the
optimizer tail) are complete, the buffer rotations (``dXt`` / ``dXi`` / ``DF_`` in threes, ``T_`` / ``I_`` by layer parity) are
sufficient, and the capture reproduces those edges.  The invariant is "same kernels, same order: bit-identical to the
sequential step".  On the 2-layer, 128-wide models of the other test files a kernel lasts microseconds and the side stream has
finished before the main stream reaches the next launch, so a missing edge cannot show there.  Here:

1. every schedule (fused ``forward_backward`` + ``Adam.step``, eager two-stream, graph with either or both overlaps) against the
   one-stream sequential step, in lockstep over seven steps on three batches (ragged / all ones / a row with a single valid
   token; every ordered pair of batches follows each other once), ``torch.equal`` after every step on parameters, 16-bit shadow,
   both Adam moments, gradients, logits, the correct count and the loss -- config 3 at B = 32, S = 128 in fp16 (with an
   overflowing step in the middle) and bf16, dense text rows, the reference's dropout, the global clip, the three
   ``skip_nonfinite`` settings, config 5's widths at 4 + 4 layers, and small models whose towers differ in depth both ways;
2. the same equality for the eager two-stream schedule with ONE STREAM MADE LATE on purpose (a bounded ``torch.cuda._sleep`` put
   on the side stream in front of every segment's weight-gradient GEMMs, or on the main stream behind every segment; sized from
   the measured step time so the late stream lags by about a whole step): timing no longer decides whether a missing edge shows;
3. the unequal-depth models over three training steps against the CPU oracle, with the bounds of
   ``test_model_gpu.py::test_tiny_step_matches_oracle_and_golden`` (fp16: logits within 1e-3, as ``test_model_fp16_gpu.py``).

A graph schedule that ran eagerly would prove nothing: ``GraphedStep`` falls back to eager launches once RCCL communicators have
been destroyed in the process (``ddp.communicator_was_destroyed()``), and in a whole-suite run ``test_model_gpu.py`` has created and
destroyed one before this file starts.  Every graph schedule therefore asserts ``use_graph`` and ``graphs is not None``, and when
the pytest process has a destroyed communicator behind it (``_graphs_replayable``) the case runs in a fresh child process, one at a
time, each under its own time limit.
"""
import os
import subprocess
import sys
import time

import pytest
import torch
from conftest import parity_log

pytestmark = pytest.mark.gpu

LR = 2e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_ENV = "MEMEHIP_SCHEDULE_TEST_CHILD"                    # set for the child process of _run_in_child
FORCE_CHILD_ENV = "MEMEHIP_SCHEDULE_TEST_FORCE_CHILD"        # = 1: take the child-process route even where graphs still replay here
# every ordered pair of the three batches occurs once as (previous step, this step)
BATCH_ORDER = (0, 1, 2, 1, 0, 2, 0)
OVERFLOW_STEP = 3


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import multimodal_propaganda_meme_classification_amd as m
    return m


def _oracle():
    from oracle import meme_oracle as O
    return O


# ---- configurations -----------------------------------------------------------------------------------------------------------

def _unequal(O, text_layers, image_layers):
    return O.OracleConfig(
        text=O.TextConfig(vocab_size=512, hidden=128, layers=text_layers, heads=2, intermediate=256, max_position=64, type_vocab=2),
        image=O.ImageConfig(image_size=32, patch=16, hidden=128, layers=image_layers, heads=2, intermediate=256),
        proj=128, num_classes=2, pool="cls")


def _case(name):
    """name -> dict(cfg (oracle config), B, S, dtype, pack, dropout, clip, skip, overflow, seed)"""
    O = _oracle()
    c = dict(cfg=None, B=32, S=128, dtype="fp16", pack=True, dropout=False, clip=None, skip=None, overflow=False, seed=31)
    if name.startswith("config3"):
        c["cfg"] = O.config3("cls")
        kind = name[len("config3-"):]
        if kind == "fp16":
            c["overflow"] = True          # an inf pixel in the middle step, as tests/test_scaler_gpu.py does
        elif kind == "bf16":
            c["dtype"] = "bf16"
        elif kind == "dense":
            c["pack"] = False
        elif kind == "dropout":
            c["dropout"] = True
        elif kind == "clip1":
            c["clip"] = 1.0
        elif kind.startswith("skip-"):
            c["skip"] = {"true": True, "false": False, "strict": "strict"}[kind[5:]]
        else:
            raise ValueError(name)
    elif name == "config5-4layers":
        c.update(cfg=O.config5("cls", layers=4), S=256)
    elif name == "text5-image2":
        c.update(cfg=_unequal(O, 5, 2), B=5, S=23)        # neither a tile multiple
    elif name == "text2-image5":
        c.update(cfg=_unequal(O, 2, 5), B=5, S=23)
    else:
        raise ValueError(name)
    return c


_PARAMS = {}


def _params(O, cfg, seed):
    """The oracle's seeded "pretrained-like" state dict; the last one is kept (every model of a case loads the same one)."""
    key = (repr(cfg), seed)
    if key not in _PARAMS:
        _PARAMS.clear()
        _PARAMS[key] = O.init_params(cfg, seed)
    return _PARAMS[key]


def _model(pkg, O, c):
    d = c["cfg"].to_dict()
    mc = pkg.ModelConfig.from_dict(d)
    if c["cfg"] == O.config3("cls"):
        assert mc == pkg.ModelConfig(), "config 3 is ModelConfig() itself, what bench.py builds"
    mc.compute_dtype = c["dtype"]
    mc.pack_text = c["pack"]
    if c["dropout"]:
        mc.with_reference_dropout()
    model = pkg.MultimodalClassifier.from_config(mc, init=False)
    model.load_state_dict(_params(O, c["cfg"], c["seed"]))
    model.to("cuda").train()
    model.manual_seed(1234)          # every model of a case draws the same dropout masks: same seed, same step counter
    return model


def _batches(O, c):
    """Three batches: ragged; all ones; ragged with one row of a single valid token (so three different live-row counts)."""
    cfg, B, S = c["cfg"], c["B"], c["S"]
    b0 = O.synthetic_batch(cfg, B, S, seed=101)
    b1 = O.synthetic_batch(cfg, B, S, seed=102, all_ones_mask=True)
    text, image, mask, labels = O.synthetic_batch(cfg, B, S, seed=103)
    mask[0, 1:] = 0
    text[0, 1:] = 0
    b2 = (text, image, mask, labels)
    live = [int(b[2].sum()) for b in (b0, b1, b2)]
    assert len(set(live)) == 3 and live[1] == B * S and int(b2[2][0].sum()) == 1, live
    return [[t.cuda() for t in b] for b in (b0, b1, b2)], live


# ---- one schedule = a model, its optimizer and a way to run one step ------------------------------------------------------------

class _Schedule:
    def __init__(self, pkg, O, c, name, fused=False, **step_kw):
        self.name, self.fused = name, fused
        self.model = _model(pkg, O, c)
        self.opt = pkg.Adam(self.model.parameters(), lr=LR, model=self.model, max_grad_norm=c["clip"], skip_nonfinite=c["skip"])
        self.B, self.S = c["B"], c["S"]
        self.step, self.scaler, self.graph = None, None, False
        if fused:
            # what GraphedStep sets up by itself: an fp16 model whose optimizer guards against non-finite gradients gets the
            # device-resident dynamic loss scale
            if c["dtype"] == "fp16" and c["skip"] is not False:
                self.scaler = pkg.GradScaler()
                self.scaler.attach_model(self.model)
        else:
            self.step = pkg.GraphedStep(self.model, self.opt, self.B, self.S, **step_kw)
            self.scaler = self.step.scaler
        self.loss = None

    def run(self, batch):
        if self.fused:
            self.loss, _, _ = self.model.forward_backward(*batch)
            if self.scaler is not None:
                self.scaler.step(self.opt)
                self.scaler.update()
            else:
                self.opt.step()
        else:
            self.step.load_batch(*batch)
            self.loss, _ = self.step.step()

    def plan(self):
        return self.step.plan if self.step is not None else self.model._get_engine().plan(self.B, self.S, True)

    def tensors(self):
        f, p = self.opt._flat, self.plan()
        return dict(flat_params=self.model.flat_params, flat_shadow=self.model.flat_shadow, adam_m=f["M"], adam_v=f["V"],
                    flat_grads=self.model.flat_grads, logits=p.buf["logits"], ncorrect=p.buf["ncorrect"], loss=self.loss)

    def close(self):
        if self.step is not None:
            self.step.close()
        self.step = self.model = self.opt = self.scaler = self.loss = None


def _same(a, b, nan_is_data):
    if torch.equal(a, b):
        return True
    if not nan_is_data or not a.is_floating_point():
        return False
    # the overflowing step: gradients / logits / loss are nan by construction (nan != nan under torch.equal); nan at the same
    # places and equal everywhere else is what "the same numbers" means there
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _where(key, a, b, layout):
    """Name the part of a flat buffer that differs: element range, layer range, first parameter."""
    ne = (a != b) & ~(torch.isnan(a) & torch.isnan(b)) if a.is_floating_point() else (a != b)
    idx = torch.nonzero(ne.reshape(-1))
    n, lo, hi = int(idx.numel()), int(idx.min()), int(idx.max())
    msg = f"{n} of {a.numel()} elements differ, flat [{lo}, {hi}]"
    if key in ("flat_params", "flat_shadow", "adam_m", "adam_v", "flat_grads"):
        layers = [l for l, s, e in layout.layer_ranges if s <= hi and lo < e]
        first = [sp.name for sp in layout.specs if sp.offset <= lo < sp.offset + sp.numel]
        msg += f"; matrix slices of layers {layers if layers else 'none (tail: head, biases, LayerNorms, embeddings)'}"
        msg += f"; first differing parameter {first[0] if first else '?'}"
        d = (a.reshape(-1)[lo].item(), b.reshape(-1)[lo].item())
        msg += f"; there: got {d[0]!r}, sequential {d[1]!r}"
    return msg


def _compare(ref, other, step, layout, nan_is_data, tag):
    tr, to = ref.tensors(), other.tensors()
    n = 0
    for key, a in to.items():
        b = tr[key]
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, other.name, key)
        if not _same(a, b, nan_is_data):
            pytest.fail(f"[{tag}] schedule '{other.name}' differs from the sequential step in {key} after step {step}: "
                        + _where(key, a, b, layout), pytrace=False)
        n += a.numel()
    return n


def _lockstep(pkg, name, schedules_fn, tag, before_step=None):
    """Drive the sequential reference and every schedule `schedules_fn` builds over BATCH_ORDER; compare after every step."""
    O = _oracle()
    c = _case(name)
    torch.set_num_threads(16)
    t_start = time.time()
    ref = _Schedule(pkg, O, c, "sequential", use_graph=False, overlap_wgrad=False, overlap_optimizer=False)
    everyone = [ref]
    try:
        assert ref.step.side is None and not ref.step.opt_in_bwd and not ref.step.use_graph
        others = schedules_fn(O, c)
        everyone += others
        layout = ref.model.layout
        batches, live = _batches(O, c)
        if c["overflow"]:
            bad = [t.clone() for t in batches[BATCH_ORDER[OVERFLOW_STEP]]]
            bad[1][1, 0, 3, 3] = float("inf")
        elements = 0
        for step, bi in enumerate(BATCH_ORDER):
            overflow = c["overflow"] and step == OVERFLOW_STEP
            batch = bad if overflow else batches[bi]
            if overflow:
                before = [(s.model.flat_params.clone(), s.opt._flat["M"].clone(), s.opt._flat["V"].clone(), s.model.flat_shadow.clone())
                          for s in everyone]
            for s in everyone:
                if before_step is not None:
                    before_step(s)
                s.run(batch)
                if before_step is not None:
                    before_step(None)
            torch.cuda.synchronize()
            for s in others:
                if s.step is not None and s.graph:
                    assert s.step.use_graph and s.step.graphs is not None, f"'{s.name}' did not replay a hipGraph: the comparison would prove nothing"
                elements += _compare(ref, s, step, layout, overflow, tag)
            if overflow:
                for s, (p0, m0, v0, sh0) in zip(everyone, before):
                    assert torch.equal(s.model.flat_params, p0) and torch.equal(s.opt._flat["M"], m0) and torch.equal(s.opt._flat["V"], v0) \
                        and torch.equal(s.model.flat_shadow, sh0), f"'{s.name}': the overflowing step changed parameters / moments / shadow"
                    assert s.opt.last_step_skipped, s.name
                assert not bool(torch.isfinite(ref.model.flat_grads).all()), "the inf pixel did not reach the gradients"
            else:
                assert bool(torch.isfinite(ref.model.flat_params).all()) and bool(torch.isfinite(ref.loss).all()), step
        if c["overflow"]:
            for s in everyone:
                assert s.opt.skipped_steps == 1, (s.name, s.opt.skipped_steps)
                # GradScaler(): initial scale 1, one overflow halves it, 2000 clean steps would be needed to grow
                assert s.scaler is not None and s.scaler.get_scale() == 0.5, (s.name, s.scaler.get_scale())
        else:
            assert all(s.opt.skipped_steps == 0 for s in everyone if s.opt._accounted)
        parity_log(f"[{tag}] {len(BATCH_ORDER)} steps x {len(others)} schedules ({', '.join(s.name for s in others)}) == sequential: "
                   f"{elements} elements compared bit for bit; live text rows per batch {live}; {time.time() - t_start:.1f} s")
    finally:
        for s in everyone:
            s.close()
        del everyone[:]
        ref = others = None
        import gc
        gc.collect()
        torch.cuda.empty_cache()


# ---- 1. every schedule against the sequential step ----------------------------------------------------------------------------------

def _all_schedules(pkg, name):
    def build(O, c):
        out = []
        for nm, fused, graph, kw in (
                ("fused", True, False, {}),
                ("eager two-stream", False, False, dict(use_graph=False)),
                ("graph, wgrad overlap only", False, True, dict(use_graph=True, overlap_optimizer=False)),
                ("graph, optimizer overlap only", False, True, dict(use_graph=True, overlap_wgrad=False)),
                ("graph, both", False, True, dict(use_graph=True))):
            s = _Schedule(pkg, O, c, nm, fused=fused, **kw)
            s.graph = graph
            out.append(s)
        both, eager2 = out[4].step, out[1].step
        # what each optimizer setting implies for the overlaps (model.GraphedStep.__init__)
        want_opt_in_bwd = c["clip"] is None and c["skip"] != "strict"
        for g in (both, eager2):
            assert g.side is not None and g.wgrad_side, "the weight-gradient overlap must be on"
            assert g.opt_in_bwd == want_opt_in_bwd, (name, g.opt_in_bwd)
        assert not out[2].step.opt_in_bwd and not out[3].step.wgrad_side and out[3].step.opt_in_bwd == want_opt_in_bwd
        if c["dtype"] == "fp16":
            resolved = {None: True, True: True, False: False, "strict": "strict"}[c["skip"]]
            assert all(s.opt.skip_nonfinite == resolved for s in out if not s.fused)
            assert all((s.scaler is not None) == (c["skip"] is not False) for s in out)
        assert both.plan.packed == c["pack"] and getattr(both.plan, "dropout_on", False) == c["dropout"]
        return out
    return build


def _graphs_replayable():
    """May this process still capture and replay multi-stream hipGraphs?  Not once an RCCL communicator has been destroyed in it.
    The product's own guard (ddp.communicator_was_destroyed()) tolerates ONE create / destroy cycle, which is what a whole-suite run
    has behind it when this file starts (tests/test_model_gpu.py's module-scoped group).  At the sizes of this file that one cycle
    was enough: the first whole-suite run with these tests in the pytest process died inside hipGraphLaunch while replaying a
    config-3 step (the fault of profiles/r04_segfault_record.md; recorded in profiles/r11_step_schedules.txt).  So the rule here is
    stricter than the product's: any destroyed communicator sends the graph cases to a fresh process."""
    import torch.distributed as dist
    from multimodal_propaganda_meme_classification_amd import ddp
    alive = dist.is_available() and dist.is_initialized()
    return ddp._DESTROYED == 0 and not (ddp._SEEN_GROUP and not alive) and not ddp.communicator_was_destroyed()


def _run_in_child(nodeid, seconds):
    """The pytest process can no longer replay hipGraphs (an RCCL communicator was destroyed in it): run this one test in a fresh
    process, wait for it, hand its output on."""
    env = dict(os.environ)
    env[CHILD_ENV] = "1"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", nodeid, "-q", "-x", "-s", "-p", "no:cacheprovider"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=seconds)
    tail = out.stdout[-6000:] + out.stderr[-3000:]
    print(tail)
    assert out.returncode == 0 and " passed" in out.stdout, f"child process for {nodeid} failed (rc {out.returncode}):\n{tail}"


SLOW = pytest.mark.slow
LOCKSTEP_CASES = [
    pytest.param("config3-fp16", id="config3-fp16"),              # what bench.py times, with an overflowing step in the middle
    pytest.param("config3-dropout", id="config3-dropout"),
    pytest.param("config3-clip1", id="config3-clip1"),
    pytest.param("text5-image2", id="text5-image2"),
    pytest.param("text2-image5", id="text2-image5"),
    pytest.param("config3-bf16", id="config3-bf16", marks=SLOW),
    pytest.param("config3-dense", id="config3-dense", marks=SLOW),
    pytest.param("config3-skip-true", id="config3-skip-true", marks=SLOW),
    pytest.param("config3-skip-false", id="config3-skip-false", marks=SLOW),
    pytest.param("config3-skip-strict", id="config3-skip-strict", marks=SLOW),
    pytest.param("config5-4layers", id="config5-4layers", marks=SLOW),
]


@pytest.mark.parametrize("name", LOCKSTEP_CASES)
def test_every_schedule_equals_the_sequential_step(pkg, request, name):
    """Fused, eager two-stream and the three graph schedules against the one-stream sequential step: parameters, shadow, moments,
    gradients, logits, correct count and loss bit-identical after each of seven steps (module docstring, part 1)."""
    in_child = os.environ.get(CHILD_ENV) == "1"
    if not in_child and (not _graphs_replayable() or os.environ.get(FORCE_CHILD_ENV) == "1"):
        _run_in_child(f"{request.node.path}::{request.node.name}", 900)
        return
    _lockstep(pkg, name, _all_schedules(pkg, name), f"schedules {name}")


# ---- 2. one stream made late on purpose -------------------------------------------------------------------------------------------------

class _Delay:
    """A bounded device-side delay: torch.cuda._sleep (a spin on the device clock), calibrated against events; where this build
    has no _sleep, repeated in-place adds on a 256-MB buffer (a harmless kernel of measured length)."""

    def __init__(self):
        self.buf = None
        self.sleep = getattr(torch.cuda, "_sleep", None)
        unit = 100_000 if self.sleep is not None else 1
        if self.sleep is None:
            self.buf = torch.zeros(64 << 20, device="cuda")
        self._issue(unit)
        for _ in range(24):                    # double until the unit lasts >= 1 ms (at most a few ms are ever spent here)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._issue(unit)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 1.0:
                break
            unit *= 2
        assert ms >= 1.0, "could not calibrate the delay kernel"
        self.per_ms = unit / ms

    def _issue(self, units):
        if self.sleep is not None:
            self.sleep(int(units))
        else:
            for _ in range(int(units)):
                self.buf.add_(1.0)

    def issue(self, ms, stream):
        assert 0.0 < ms < 500.0, ms             # bounded: never more than half a second per call
        with torch.cuda.stream(stream):
            self._issue(max(1, round(ms * self.per_ms)))


def _time_sequential_step(pkg, O, c):
    """Median of three steps of the sequential schedule on a model of its own (after one warm-up step), in ms."""
    s = _Schedule(pkg, O, c, "timer", use_graph=False, overlap_wgrad=False, overlap_optimizer=False)
    try:
        batches, _ = _batches(O, c)
        ms = []
        for k in range(4):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.run(batches[k % 3])
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        n_bwd = len(s.step.plan.bwd)
        return sorted(ms[1:])[1], n_bwd
    finally:
        s.close()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("late", ["late-side", "late-main"])
@pytest.mark.parametrize("name", ["config3-fp16", "config3-dropout", "text5-image2", "text2-image5"])
def test_eager_two_stream_with_one_stream_made_late(pkg, monkeypatch, name, late):
    """The eager two-stream schedule (the host issues every launch; Segment.run2 places the cross-stream edges) with a delay on
    one stream around every backward segment that forks weight-gradient GEMMs:
      late-side: the side stream sleeps BEFORE the segment's lane-1 work, so the weight-gradient GEMMs and the Adam slice behind
                 them start when the main stream is well into the layers below -- a buffer the main chain overwrites without
                 having waited, or an optimizer tail that reads gradients too early, changes numbers;
      late-main: the main stream sleeps AFTER the segment has been issued, so the side stream's GEMMs and Adam slice finish long
                 before the main chain moves on.
    Latency only: launch arguments and launch order are untouched, the graph path is not involved.  The delay per segment is the
    measured sequential step time divided by the number of delayed segments (at least step time / backward segments), so the
    late stream lags by about a whole step.  The result must still equal the sequential step bit for bit (module docstring, part 2)."""
    from multimodal_propaganda_meme_classification_amd import engine
    O = _oracle()
    c = _case(name)
    torch.set_num_threads(16)
    step_ms, n_bwd = _time_sequential_step(pkg, O, c)
    delay = _Delay()
    state = dict(active=False, issued=0)
    orig = engine.Segment.run2

    def run2(self, main, side, events):
        forks = state["active"] and side is not None and any(call[5] == 1 and call[0] is not None for call in self.calls)
        if forks and late == "late-side":
            delay.issue(state["ms"], side)
            state["issued"] += 1
        orig(self, main, side, events)
        if forks and late == "late-main":
            delay.issue(state["ms"], main)
            state["issued"] += 1

    monkeypatch.setattr(engine.Segment, "run2", run2)

    def build(O_, c_):
        s = _Schedule(pkg, O_, c_, f"eager two-stream, {late}", use_graph=False)
        s.graph = False
        assert s.step.side is not None and s.step.wgrad_side and s.step.opt_in_bwd and not s.step.use_graph
        n_fork = sum(1 for sg in s.step.plan.bwd if any(call[5] == 1 for call in sg.calls))
        assert 0 < n_fork <= n_bwd
        state["ms"] = step_ms / n_fork            # >= step_ms / n_bwd
        state["n_fork"] = n_fork
        return [s]

    def before_step(s):
        state["active"] = s is not None and s.name.startswith("eager two-stream")

    tag = f"{late} {name}"
    _lockstep(pkg, name, build, tag, before_step=before_step)
    assert state["issued"] == state["n_fork"] * len(BATCH_ORDER), state
    parity_log(f"[{tag}] sequential step {step_ms:.3f} ms, {n_bwd} backward segments; {state['ms']:.3f} ms injected on the "
               f"{'side' if late == 'late-side' else 'main'} stream at each of the {state['n_fork']} segments that fork weight-gradient GEMMs "
               f"({state['ms'] * state['n_fork']:.3f} ms per step, {state['issued']} delays in all; "
               f"{'torch.cuda._sleep' if delay.sleep is not None else 'add_ kernels'}, {delay.per_ms:.0f} units per ms)")


# ---- 3. the unequal-depth models against the oracle ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("text_layers,image_layers", [(5, 2), (2, 5)])
def test_unequal_depth_three_steps_match_the_oracle(pkg, text_layers, image_layers, dtype):
    """The has_t / has_i branches of the launch plan (one tower deeper than the other, both ways) over three training steps against
    the CPU oracle: logits, loss, every parameter's gradient, parameters after each step -- the loop and the bounds of
    test_model_gpu.py::test_tiny_step_matches_oracle_and_golden (logits: 3e-3 * sqrt(layers / 2) in bf16, 1e-3 in fp16 as in
    test_model_fp16_gpu.py; gradients 3e-2 relative per tensor; parameters 2.05 * k * lr per element and 0.05 * lr in the mean)."""
    from test_model_gpu import _grad_check, logit_tol_bf16
    O = _oracle()
    cfg = _unequal(O, text_layers, image_layers)
    params = O.init_params(cfg, 17)
    d = cfg.to_dict()
    d["compute_dtype"] = dtype
    model = pkg.MultimodalClassifier.from_config(pkg.ModelConfig.from_dict(d), init=False)
    model.load_state_dict(params)
    model.to("cuda").train()
    text, image, mask, labels = O.synthetic_batch(cfg, 5, 23, seed=19)
    opt = pkg.Adam(model.parameters(), lr=LR)
    crit = pkg.CrossEntropyLoss()
    st = O.AdamState()
    p_ref = params
    tag = f"[oracle, text {text_layers} / image {image_layers} layers, {dtype}]"
    for step in range(3):
        opt.zero_grad()
        output = model(text.cuda(), image.cuda(), mask.cuda())
        loss = crit(output, labels.cuda())
        loss.backward()
        p_next, ref_logits, ref_loss, ref_grads = O.train_step(p_ref, st, text, image, mask, labels, cfg, lr=LR)
        got = output.detach().float().cpu()
        tol = logit_tol_bf16(O, p_ref, text, image, mask, cfg, ref_logits) if dtype == "bf16" else 1e-3
        err, lerr = float((got - ref_logits).abs().max()), abs(float(loss.detach()) - float(ref_loss))
        gname, gworst = "", 0.0
        for nm, p in model.named_parameters():            # measured before it is asserted
            if ".key.bias" not in nm:
                r = float((p.grad.detach().float().cpu() - ref_grads[nm]).norm()) / (float(ref_grads[nm].norm()) + 1e-12)
                if r > gworst:
                    gname, gworst = nm, r
        parity_log(f"{tag} step {step}: max |logit - oracle| = {err:.3e} (bound {tol:.3e}), |loss - oracle| = {lerr:.3e}, "
                   f"worst gradient ||diff|| / ||ref|| = {gworst:.3e} ({gname}; bound 3e-2)")
        assert err <= tol, (step, tol, got, ref_logits)
        assert lerr <= tol
        _grad_check(model, ref_grads)
        opt.step()
        p_ref = p_next
        sd = model.state_dict()
        tot, cnt, worst = 0.0, 0, 0.0
        for k, ref in p_ref.items():
            dd = (sd[k].detach().float().cpu() - ref).abs()
            worst = max(worst, float(dd.max()))
            if ".key.bias" not in k:
                tot += float(dd.sum()); cnt += dd.numel()
        parity_log(f"{tag} step {step}: parameters max |diff| = {worst:.3e} (bound {2.05 * (step + 1) * LR:.3e}), "
                   f"mean |diff| = {tot / cnt:.3e} (bound {0.05 * LR:.3e})")
        for k, ref in p_ref.items():
            dd = (sd[k].detach().float().cpu() - ref).abs()
            assert float(dd.max()) <= 2.05 * (step + 1) * LR, (k, float(dd.max()))
        assert tot / cnt < 0.05 * LR, tot / cnt
