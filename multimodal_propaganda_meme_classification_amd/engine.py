"""Launch plan of one fine-tune step: which HIP kernels run, on which buffers, in which order.

A ``Plan`` is built once per (batch, seq_len): every activation / gradient workspace is allocated
up front (288 GB of HBM: nothing is recomputed, nothing is freed) and every kernel launch is
recorded as a prepared C-ABI call.  Running a step is then a replay of prepared calls -- eagerly,
or captured once into a hipGraph (model.GraphedStep) so the ~220 launches cost one host call.

The two towers run in LOCKSTEP: layer l of the text encoder and layer l of the image encoder
issue the same kernel sequence, so every launch is a *grouped* launch carrying both towers'
problems: GEMMs (forward, dgrad; the weight gradients as one launch per tower), LayerNorms and
attention.  That is what fills 256 CUs at these sizes (768-wide projections give only 100-300
128x128 tiles per tower).  The text tower is padding-free: its launches are sized for B*S rows and
clamp themselves to the live row count on the device (see the "pk.*" buffers in _build).

Reference for the math: BertModel / timm ViT as called at
example_scripts/Multimodal_example_task2C.txt:175,183 and the step at :200-223.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import (MH_GEMM_ACCUM, MH_GEMM_DERIV_AUX, MH_GEMM_GELU, MH_GEMM_OUT_F32, MH_GEMM_QUICK_GELU, MhAttnProblem, MhColsumJob, MhGemmProblem,
                   MhHeadGrads, MhHeadParams, MhLnBwdJob, MhLnFwdJob, MhRowsJob, MhSpanJob)
from .config import Layout, ModelConfig, check_sequence_length

BF16, F32, I64 = torch.bfloat16, torch.float32, torch.int64
LN_PARTS = 512     # workgroups (= sets of dgamma/dbeta partials) per LayerNorm backward

LAUNCH, PY, WAIT = "launch", "py", "wait"


class Call(NamedTuple):
    """One entry of a Segment.  A launch has ``fn``; the two other kinds carry their payload in ``args``."""
    fn: Optional[Callable]      # prepared C-ABI entry point (called as fn(*args, stream)); None unless kind == LAUNCH
    args: object                # LAUNCH: the argument tuple; PY: a python callback; WAIT: the name of the segment to wait for
    name: str                   # C-ABI function name (error messages)
    tag: str                    # kernel family, for run_timed
    work: object                # FLOPs or bytes of the launch: a float, or (fixed, per-live-row part at the maximum row count)
    lane: int                   # 1 = a weight-gradient GEMM, which nothing later in the backward chain reads
    kind: str = LAUNCH


class Segment:
    """An ordered list of prepared launches."""

    def __init__(self, name: str, lib=None):
        self.name = name
        self.lib = lib if lib is not None else _lib.load()
        self.calls: List[Call] = []

    def c(self, fn_name: str, *args, tag: Optional[str] = None, work: float = 0.0, lane: int = 0):
        self.calls.append(Call(getattr(self.lib, fn_name), args, fn_name, tag or fn_name, work, lane))

    def py(self, fn: Callable[[], None]):
        self.calls.append(Call(None, fn, PY, PY, 0.0, 0, PY))

    def wait(self, key: str):
        """On a multi-stream run: the main stream waits for the lane-1 work of segment `key`."""
        self.calls.append(Call(None, key, WAIT, WAIT, 0.0, 0, WAIT))

    def run(self, stream: int):
        for fn, args, name, _, _, _, kind in self.calls:
            if fn is None:
                if kind == PY:
                    args()
            else:
                st = fn(*args, stream)
                if st != 0:
                    _lib.check(st, name)

    def run2(self, main: "torch.cuda.Stream", side: Optional["torch.cuda.Stream"], events: Dict[str, "torch.cuda.Event"]):
        """Two-stream replay (single GPU).  lane 1 = the weight-gradient GEMMs, which nothing later in the backward
        chain reads: they go to `side`, forked behind everything issued so far on `main`, and their completion event
        is stored under this segment's name for a later wait().  (A third stream for the image tower's LayerNorm /
        attention beside the text tower's was measured slower -- the cross-stream edges cost more than the overlap of
        those short kernels returned -- and removed; both towers now share grouped launches instead.)"""
        mp = main.cuda_stream
        sp = side.cuda_stream if side is not None else mp      # side=None: lane-1 work stays on the main stream
        forked1 = False
        for fn, args, name, _, _, lane, kind in self.calls:
            if fn is None:
                if kind == PY:
                    args()
                elif kind == WAIT:
                    if args in events:
                        main.wait_event(events.pop(args))
                continue
            if lane == 1 and side is not None:
                if not forked1:
                    e = torch.cuda.Event()
                    e.record(main)
                    side.wait_event(e)
                    forked1 = True
                st = fn(*args, sp)
            else:
                st = fn(*args, mp)
            if st != 0:
                _lib.check(st, name)
        if forked1:
            d = torch.cuda.Event()
            d.record(side)
            events[self.name] = d

    def run_timed(self, stream: int, tag: str, out: list, dyn_scale: float = 1.0):
        """Eager replay that brackets every launch tagged `tag` with events on the launch stream;
        appends (start_event, end_event, work) to `out`.  `work` of a launch is (fixed, per-live-row part at the
        maximum row count): dyn_scale = live rows / maximum rows of the packed text tower."""
        for fn, args, name, t, work, _, kind in self.calls:
            if isinstance(work, tuple):
                work = work[0] + work[1] * dyn_scale
            if fn is None:
                if kind == PY:
                    args()
                continue
            if t == tag:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                st = fn(*args, stream)
                e1.record()
                out.append((e0, e1, work))
            else:
                st = fn(*args, stream)
            if st != 0:
                _lib.check(st, name)

    def __len__(self):
        return len(self.calls)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


class LossOptions(NamedTuple):
    """The scalar options of the fused step's loss (mh_ce_opts_fwd_bwd); hashable: part of a plan's key.  The class-weight VALUES are not
    part of it -- they live in one device buffer and may change under a built (or captured) plan -- only whether there are any."""
    weighted: bool
    ignore_index: Optional[int]
    label_smoothing: float
    reduction: str              # "mean" | "sum"


class Plan:
    def __init__(self, B: int, S: int, lib=None):
        self.B, self.S = B, S
        self.lib = lib
        self.buf: Dict[str, torch.Tensor] = {}
        self.keep: list = []                  # ctypes arrays referenced by prepared calls
        self.fwd = Segment("fwd", lib)
        self.loss = Segment("loss", lib)
        self.bwd: List[Segment] = []          # backward segments in execution order
        # gradient accumulation: the same backward over the same activations and temporaries, ADDING into the flat gradient buffer
        # (built on first use by Engine.add_flavour, from the arguments the plan was built with; None until then).  The plan keeps
        # no reference to its builder: a plan must die with its engine by reference count alone -- it owns the activations.
        self.bwd_add: Optional[List[Segment]] = None
        self.build_args: Optional[tuple] = None
        self.bucket_after: Dict[str, Tuple[int, int]] = {}   # segment name -> flat grad range complete after it
        self.n_launches = 0
        self.gemm_flops = 0.0                 # algorithmic GEMM FLOPs of one step (fwd + dgrad + wgrad), no row packed away
        self.gemm_flops_dyn = 0.0             # the part of it that scales with the live rows of the packed text tower
        self.packed = False
        self.dropout_on = False               # some dropout probability is non-zero in this plan
        self.features = False                 # False | True | "sequence": where the plan stops (Engine.plan)
        self.loss_opts = None                 # the LossOptions the loss launch was built with (None: mh_ce_fwd_bwd)
        self.last_rows = "all"                # "pooled": the blocks behind the last attention run on the B pooled rows only
        self.gather = None                    # data parallel: (local, gathered) tensor pairs exchanged before "bwd_embed_tables"
        self._ln_jobs: Dict[int, list] = {}   # width -> (partials, dgamma, dbeta) of every LayerNorm backward, summed in "bwd_embed"


class Engine:
    def __init__(self, cfg: ModelConfig, layout: Layout, P: torch.Tensor, G: torch.Tensor, SH: torch.Tensor):
        self.cfg, self.layout = cfg, layout
        self.P, self.G, self.SH = P, G, SH
        self.dev = P.device
        assert P.is_cuda and G.is_cuda and SH.is_cuda, "memehip needs HIP device buffers (no CPU fallback)"
        self.kind = cfg.compute_dtype
        self.T16 = torch.float16 if self.kind == "fp16" else torch.bfloat16
        assert SH.dtype == self.T16
        self.lib = _lib.load(self.kind)
        self.gscale = cfg.stream_scale          # scale carried by the 16-bit gradient streams
        self.pack_text = cfg.pack_text          # padding-free text tower (rows with attention_mask == 0 are never computed)
        self.plans: Dict[Tuple[int, int], Plan] = {}
        # one byte per word-embedding row: has it ever received a gradient?  (rows that have not keep g = m = v = 0,
        # for which Adam is the identity: model.Adam skips them, mh_adam_step_rows)
        self.word_row_live = torch.zeros(cfg.text.vocab_size, dtype=torch.uint8, device=self.dev)
        # id index of the embedding-gradient kernel (first position / multiplicity per vocabulary row; self-restoring)
        self.word_first = torch.full((cfg.text.vocab_size,), 0x7fffffff, dtype=torch.int32, device=self.dev)
        self.word_count = torch.zeros(cfg.text.vocab_size, dtype=torch.int32, device=self.dev)
        # dynamic loss scale read by the fused loss launch (1 = none; a memehip.GradScaler attached to the model owns it)
        self.loss_scale = torch.ones(1, dtype=F32, device=self.dev)
        # the fused step's loss (model.set_loss_options): None = the plain mean cross-entropy (mh_ce_fwd_bwd); otherwise a LossOptions,
        # part of every plan's key, and the model-owned class-weight buffer the loss launch of such plans points at
        self.loss_opts: Optional[LossOptions] = None
        self.class_weight: Optional[torch.Tensor] = None
        # gradient accumulation over micro-batches (model.set_grad_accumulation): a scratch mirror of the small gradients' run of the
        # flat buffer (n_shadow .. the word table; allocated on first use) and the token ids of every ADDING backward of the
        # current window, whose word-table rows the first backward of the next window has to clear
        self.small0 = layout.n_shadow
        self.small1 = layout.spec[WORD_TABLE].offset
        self._mirror: Optional[torch.Tensor] = None
        self._window_ids: List[torch.Tensor] = []
        # bert position scheme: a backward writes the first S rows of the position-table gradient only; the leading rows that may
        # be non-zero.  An overwriting backward under a shorter sequence clears the rest (before_backward).
        self._pos_rows = 0

    # ---- parameter / gradient views -----------------------------------------------------------------
    def _slice(self, flat: torch.Tensor, name: str, count: int = 1) -> torch.Tensor:
        s = self.layout.spec[name]
        return flat[s.offset:s.offset + s.numel * count]

    def p(self, name, count=1):
        return self._slice(self.P, name, count)

    def g(self, name, count=1):
        return self._slice(self.G, name, count)

    def w(self, name, count=1):
        s = self.layout.spec[name]
        assert s.offset + s.numel * count <= self.layout.n_shadow, name
        return self.SH[s.offset:s.offset + s.numel * count]

    def mirror(self) -> torch.Tensor:
        """Scratch mirror of G[small0:small1]; an adding backward writes its small gradients here (same offsets) and adds them
        into G with mh_accum_spans_f32.  Elements no kernel writes (alignment gaps) stay zero."""
        if self._mirror is None:
            self._mirror = torch.zeros(self.small1 - self.small0, dtype=F32, device=self.dev)
        return self._mirror

    def _zero_word_rows(self, ids: torch.Tensor):
        gword = self.g(WORD_TABLE)
        st = self.lib.mh_zero_rows_f32(ids.data_ptr(), gword.data_ptr(), ids.numel(), self.cfg.text.hidden,
                                       self.cfg.text.vocab_size, torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "mh_zero_rows_f32")

    def before_backward(self, plan: Plan, add: bool = False):
        """Each plan re-zeroes the word-embedding gradient rows IT touched last time (the table gradient is dense,
        only touched rows are ever non-zero).  When the previous backward ran under a different plan (another
        batch size / sequence length), clear that plan's rows first so no stale row survives the switch.
        add = True (an adding backward inside an accumulation window): nothing is cleared, whatever plan ran last -- the rows
        of every micro-batch stay until the first (overwriting) backward of the next window, which clears them here.
        Every overwriting backward, accumulating or not, also clears the rows of the position-table gradient past this plan's
        sequence length, which a longer batch (or a longer micro-batch of the window before) wrote: the absolute scheme writes
        the first S rows only.  (The roberta scheme writes every row of the table gradient itself.)"""
        if add:
            self._pos_rows = max(self._pos_rows, plan.S)
            return
        if self._pos_rows > plan.S and self.cfg.text.position_scheme != "roberta":
            D = self.cfg.text.hidden
            self.g(TXT + "embeddings.position_embeddings.weight")[plan.S * D:self._pos_rows * D].zero_()
            self._pos_rows = plan.S
        self._pos_rows = max(self._pos_rows, plan.S)
        last = getattr(self, "_last_bwd_plan", None)
        if last is not None and last is not plan:
            for key in ("prev_ids_all", "prev_ids"):
                prev = last.buf.get(key)
                if prev is not None:
                    self._zero_word_rows(prev)
                    prev.zero_()
        for ids in self._window_ids:
            self._zero_word_rows(ids)
        self._window_ids.clear()
        self._last_bwd_plan = plan

    def add_flavour(self, plan: Plan) -> List[Segment]:
        """The adding backward of `plan` (gradient accumulation): the plan's own backward, launch for launch over the same
        activations and temporaries, with the weight gradients added in the GEMM epilogue (MH_GEMM_ACCUM), the word-table rows
        added by mh_bert_embed_bwd_accum and every small gradient written to the scratch mirror and added by
        mh_accum_spans_f32 at the end.  Built on first use; the overwriting segments are untouched."""
        if plan.bwd_add is None:
            if plan.gather is not None or plan.build_args is None:
                raise ValueError("memehip: gradient accumulation is not available for a data-parallel plan (gather_world > 0)")
            # a second builder over the plan's own buffers (found by name): its forward steps only restate which buffer is what
            # (their launches are dropped), its backward steps emit the adding segments
            b = _PlanBuilder(self, *plan.build_args, add_to=plan)
            self._build_steps(b)
            assert [sg.name for sg in b.pl.bwd_add] == [sg.name for sg in plan.bwd] and not b.pl.bwd
            plan.keep.append(b.pl.keep)
            plan.bwd_add = b.pl.bwd_add
        return plan.bwd_add

    # ---- plan ----------------------------------------------------------------------------------------------
    def plan(self, B: int, S: int, training: bool = True, gather_world: int = 0, features=False,
             last_rows: str = "pooled") -> Plan:
        """Plans differ between train and eval only when some dropout probability is non-zero.
        features = True: the plan stops at the pooled tower features (text pooled row | ViT class token, f32) and its
        backward starts from their gradient: the late-fusion head is then whatever the caller builds on top.
        features = "sequence": the same with the towers' whole last hidden states ([B,S,Dt] and [B,Nt,Di], f32) as the
        boundary -- for poolings that read every position (max / mean / attention / conv1d); the reference pools over the
        padded positions too, so this plan computes them (no row packing).
        gather_world = W > 0 (data parallel): the embedding-table gradients are built from the all-gathered token ids
        and embedding-gradient rows of all W ranks (6 MB per rank) instead of all-reducing the dense 196-MB table.
        last_rows = "pooled" (default): behind the attention of each tower's last layer, only the rows the pooling reads are
        computed (see _PlanBuilder.last_layer_form); "all" computes every row.  Plans whose full last hidden states are read, or that carry
        dropout, are built as "all" whatever is asked for: ``plan.last_rows`` tells which form a plan has."""
        if last_rows not in ("pooled", "all"):
            raise ValueError(f"last_rows must be 'pooled' or 'all', got {last_rows!r}")
        cfg = self.cfg
        has_drop = (cfg.text.hidden_dropout > 0 or cfg.text.attention_dropout > 0 or cfg.head_dropout > 0)
        features = features if features == "sequence" else bool(features)
        pack = self.pack_text and features != "sequence"
        key = (B, S, bool(training and has_drop), int(gather_world), pack, features) + (() if last_rows == "pooled" else (last_rows,))
        if self.loss_opts is not None and not features:     # (no options: the key, the plan and its launches are the plain loss's)
            key += (self.loss_opts,)
        if key not in self.plans:
            self.plans[key] = self._build(B, S, key[2], key[3], key[4], key[5], last_rows=last_rows)
        return self.plans[key]

    def _build(self, B: int, S: int, dropout_on: bool = False, gather_world: int = 0, pack: bool = False,
               features=False, last_rows: str = "pooled") -> Plan:
        b = _PlanBuilder(self, B, S, dropout_on, gather_world, pack, features, last_rows)
        self._build_steps(b)
        pl = b.pl
        pl.build_args = (B, S, dropout_on, gather_world, pack, features, last_rows)
        pl.n_launches = sum(1 for sg in [pl.fwd, pl.loss] + pl.bwd for c in sg.calls if c[0] is not None)
        return pl

    @staticmethod
    def _build_steps(b: "_PlanBuilder"):
        nl = max(b.text.L, b.image.L)
        b.text_embed()
        b.image_embed()
        b.last_layer_form()
        b.layer_buffers()
        for l in range(nl):
            b.fwd_layer(l)
        b.head_and_loss()
        b.bwd_head()
        for l in range(nl - 1, -1, -1):
            b.bwd_layer(l)
        b.bwd_embed()


# ---- what a plan is built from: typed jobs, per-layer activations and gradients, one record per tower ------------------

# A dropout site: rng = pointer to int32[4] {seed_lo, seed_hi, step, -} (None = off), probability, site id.
Site = namedtuple("Site", "rng p sid", defaults=(None, 0.0, 0))
NO_DROP = Site()

# One problem of a grouped GEMM launch (MhGemmProblem); `drop` = the dropout site of the epilogue.
Gemm = namedtuple("Gemm", "A B C M N K lda ldb ldc bias residual aux mul rowsum gelu quick deriv_aux alpha drop rows_dev drop_rows accum",
                  defaults=(None, None, None, None, None, False, False, False, 1.0, NO_DROP, None, None, False))
LnFwd = namedtuple("LnFwd", "x gamma beta y mean rstd rows D eps y32 rows_dev", defaults=(None, None))
LnBwd = namedtuple("LnBwd", "dy x gamma mean rstd dx part rows D dx_add dx_drop drop rows_dev drop_rows",
                   defaults=(None, None, NO_DROP, None, None))
Attn = namedtuple("Attn", "qkv out lse B S H key_mask cu row_map drop dout delta dqkv", defaults=(None, None, None, NO_DROP, None, None, None))
# n rows of a [rows, D] buffer, named by a device index array `idx` (ascending) or as b * stride + offset
RowsJob = namedtuple("RowsJob", "n rows D idx stride offset src dst rows_dev", defaults=(None, 0, 0, None, None, None))

# Saved activations of one layer.  "rows" = the rows of everything behind its attention core ("pctx" / "x": the operands of the
# first such block, the attention output and the layer input, at those rows: gathered copies in a compact last layer).
TextActs = namedtuple("TextActs", "qkv ctx lse a y m1 r1 h g f m2 r2 pctx x rows")
ImageActs = namedtuple("ImageActs", "u m1 r1 qkv ctx lse xp w m2 r2 h g pctx x rows")

# The operands of a layer's four Linears by what they are to the GEMM (the role table of a tower, Tower.roles):
#   attn_in    input of the QKV projection                          text x_l     image u
#   proj_out   output of the attention output projection                 a            xp
#   ffn_in     input of FFN up                                           y            w
#   ffn_res    residual added to FFN down (post-LN | pre-LN)             y            xp
#   ffn_out    output of FFN down                                        f            x_{l+1}
Roles = namedtuple("Roles", "attn_in proj_out ffn_in ffn_res ffn_out")

# The gradient buffers of one layer of one tower as the blocks behind the attention core see them: the parity / rotation set of
# the layer, or in a compact last layer its [B, D] panels (res_full / dctx_full / dqkv / d_in are full size either way).
#   d_out    at the FFN-down output         text: dfm = df times its dropout mask (df itself without dropout)   image: the layer's incoming gradient
#   dh       at the GELU input
#   d_mid    at the FFN input               text: dy     image: dw
#   d_proj   at the out-proj output         text: dam = da times its dropout mask (da itself without dropout)   image: dxp
#   res      the residual branch around the attention      text: da     image: dxp
#   dctx     at the attention output
#   d_in     at the QKV input               text: the gradient at the output of the layer below                 image: du
#   df       text only: at the FFN-down output in front of its dropout = the residual branch around the FFN
Grads = namedtuple("Grads", "d_out dh d_mid d_proj res dctx res_full dctx_full dqkv d_in df", defaults=(None,))


class Tower:
    """What the lockstep schedule has to know about one encoder tower; built once per plan."""

    def __init__(self, pre, c, T, S, attn, ln_mid, post_ln, quick=False, p_h=0.0, p_a=0.0):
        self.pre, self.T, self.S = pre, T, S        # parameter-name prefix; rows of a full-size activation; sequence length
        self.D, self.I, self.H, self.L, self.eps = c.hidden, c.intermediate, c.heads, c.layers, c.ln_eps
        # the stems that differ: the fused q/k/v projection, the LayerNorm between the attention block and the FFN
        self.attn, self.ln_mid = attn, ln_mid
        self.post_ln, self.quick = post_ln, quick   # BERT: LayerNorm behind each residual sum, ViT: in front of each block; quick-GELU
        self.p_h, self.p_a = p_h, p_a               # dropout behind the two residual Linears / on the attention probabilities (BERT only)
        # padding-free text tower: live-row count and row map on the device, the packed key mask and sequence offsets
        self.rows_dev = self.row_map = self.key_mask = self.cu = None
        self.pool, self.compact = None, 0           # the rows the pooling reads (a RowsJob template); rows of the compact last layer, 0 = none
        self.x, self.acts = [], []                  # layer inputs (x[L] = the tower's last hidden state); per-layer saved activations
        self.dX, self.d_last = [], None             # gradient at a layer's output (rotation of three); the one that enters the last layer
        self.grads, self.delta = [], None           # per-layer Grads; the attention backward's row sums

    def rows(self, l: int) -> int:
        """Rows of the blocks behind the attention core of layer l."""
        return self.compact if (self.compact and l == self.L - 1) else self.T

    @property
    def out_rows(self) -> int:
        """Rows of the tower's last hidden state."""
        return self.compact or self.T

    def live(self, M: int, drop: bool = False) -> dict:
        """Clamp arguments of a GEMM problem / LayerNorm job over M rows (a [B, D] panel is never clamped by the live-row count)."""
        if self.rows_dev is None or M != self.T:
            return {}
        return dict(rows_dev=self.rows_dev, drop_rows=self.row_map) if drop else dict(rows_dev=self.rows_dev)

    def name(self, l: int, stem: str) -> str:
        return f"{self.pre}encoder.layer.{l}.{stem}"

    def roles(self, l: int) -> Roles:
        a = self.acts[l]
        return Roles(self.x[l], a.a, a.y, a.y, a.f) if self.post_ln else Roles(a.u, a.xp, a.w, a.xp, self.x[l + 1])

    def d_x(self, l: int) -> torch.Tensor:
        """Gradient at the output of layer l (l = -1: at the tower's input)."""
        return self.d_last if l == self.L - 1 else self.dX[(self.L - 1 - l) % 3]


def _fill_ln_fwd(e: MhLnFwdJob, j: LnFwd):
    assert j.x.numel() >= j.rows * j.D and j.y.numel() >= j.rows * j.D
    e.x, e.gamma, e.beta, e.y, e.y_f32 = _ptr(j.x), _ptr(j.gamma), _ptr(j.beta), _ptr(j.y), _ptr(j.y32)
    e.mean, e.rstd, e.rows, e.eps = _ptr(j.mean), _ptr(j.rstd), j.rows, j.eps
    e.rows_dev = _ptr(j.rows_dev)


def _fill_ln_bwd(e: MhLnBwdJob, j: LnBwd):
    n = j.rows * j.D
    assert j.dy.numel() >= n and j.x.numel() >= n and j.dx.numel() >= n
    assert j.dx_add is None or j.dx_add.numel() >= n
    e.dy, e.x, e.gamma, e.mean, e.rstd = _ptr(j.dy), _ptr(j.x), _ptr(j.gamma), _ptr(j.mean), _ptr(j.rstd)
    e.dx_add, e.dx, e.part, e.dx_drop, e.rng = _ptr(j.dx_add), _ptr(j.dx), _ptr(j.part), _ptr(j.dx_drop), j.drop.rng
    e.n_part, e.rows, e.drop_p, e.drop_stream = LN_PARTS, j.rows, j.drop.p, j.drop.sid
    e.rows_dev, e.drop_rows = _ptr(j.rows_dev), _ptr(j.drop_rows)


TXT, IMG = "bert.", "image_model."
WORD_TABLE = TXT + "embeddings.word_embeddings.weight"
HEAD_FIELDS = (("Wt", "bert_fc.weight"), ("bt", "bert_fc.bias"), ("Wi", "image_fc.weight"), ("bi", "image_fc.bias"),
               ("Wf", "fusion_fc.weight"), ("bf_", "fusion_fc.bias"), ("Wo", "output_fc.weight"), ("bo", "output_fc.bias"))


class _PlanBuilder:
    """Builds one Plan, step by step in execution order (Engine._build lists the steps).  What the steps share lives here:
    the plan, the two Tower records, the dropout sites and `alloc`."""

    def __init__(self, eng: Engine, B: int, S: int, dropout_on: bool, gather_world: int, pack: bool, features, last_rows: str,
                 add_to: Optional[Plan] = None):
        cfg, t, v = eng.cfg, eng.cfg.text, eng.cfg.image
        check_sequence_length(t, S)
        if B > 1024:
            raise ValueError("batch > 1024 not supported by the loss kernel")
        self.eng, self.cfg, self.B, self.S = eng, cfg, B, S
        self.T16 = eng.T16          # every 16-bit buffer uses the configured storage type
        self.pl = pl = Plan(B, S, eng.lib)
        # gradient accumulation (add_to = the plan whose adding backward is built, Engine.add_flavour): the steps run over THAT plan's
        # buffers -- `alloc` hands them back by name, what is new (a scratch of the adding flavour) joins them --, `g` gives the scratch
        # mirror for the small gradients, and the backward segments go to `pl.bwd_add`
        self.accum = add_to is not None
        if add_to is not None:
            pl.buf, pl.bwd_add = add_to.buf, []
        self.acc_spans: List[Tuple[int, int]] = []          # (flat offset, elements) written to the mirror by the adding backward
        self.acc_extra: List[Tuple[torch.Tensor, torch.Tensor]] = []      # further (destination, scratch) pairs added at its end
        self.gather_world, self.last_rows = gather_world, last_rows
        pl.dropout_on, pl.packed, pl.features = dropout_on, pack, features
        self.rng = self.alloc("rng", (4,), torch.int32, zero=True)     # the words every dropout site reads
        self.p_head = cfg.head_dropout if dropout_on else 0.0
        self.pool_index = 0 if cfg.pool == "cls" else S - 1
        self.text = Tower(TXT, t, B * S, S, "attention.self.", "attention.output.LayerNorm", post_ln=True,
                          p_h=t.hidden_dropout if dropout_on else 0.0, p_a=t.attention_dropout if dropout_on else 0.0)
        self.image = Tower(IMG, v, B * v.n_tokens, v.n_tokens, "attention.attention.", "layernorm_after", post_ln=False,
                           quick=v.act == "quick_gelu")
        self.towers = (self.text, self.image)

    def alloc(self, name, shape, dtype=None, zero=False):
        if self.accum and name in self.pl.buf:
            tns = self.pl.buf[name]
            assert tuple(tns.shape) == tuple(shape) and tns.dtype == (dtype or self.T16), name
            return tns
        tns = (torch.zeros if zero else torch.empty)(shape, dtype=dtype or self.T16, device=self.eng.dev)
        self.pl.buf[name] = tns
        return tns

    def g(self, name, count=1, written: Optional[int] = None) -> torch.Tensor:
        """Where the backward writes the gradient of `name`: its slice of the flat buffer, or, in the adding flavour, of the
        scratch mirror for everything between the GEMM matrices and the word table (`written`: the leading elements the
        backward really writes, when not all).  The matrices and the word table are added to in place."""
        eng, s = self.eng, self.eng.layout.spec[name]
        if not self.accum or not (eng.small0 <= s.offset < eng.small1):
            return eng.g(name, count)
        n = s.numel * count
        self.acc_spans.append((s.offset, n if written is None else written))
        return eng.mirror()[s.offset - eng.small0:s.offset - eng.small0 + n]

    def _accum_spans(self, s: Segment):
        """End of the adding backward: G[span] += mirror[span] for every span it wrote (adjacent ones merged; the tensors are
        16-byte aligned and padded to 4 elements, the padding is zero in the mirror), plus the extra scratch pairs."""
        eng = self.eng
        merged: List[List[int]] = []
        for off, n in sorted(set(self.acc_spans)):
            end = off + (n + 3) // 4 * 4
            if merged and off <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], end)
            else:
                merged.append([off, end])
        mir = eng.mirror()
        pairs = [(eng.G[a:min(b, eng.small1)], mir[a - eng.small0:min(b, eng.small1) - eng.small0]) for a, b in merged]
        pairs += self.acc_extra
        for i0 in range(0, len(pairs), _lib.MH_SPAN_MAX_JOBS):
            chunk = pairs[i0:i0 + _lib.MH_SPAN_MAX_JOBS]
            arr = (MhSpanJob * len(chunk))()
            for e, (dst, src) in zip(arr, chunk):
                assert dst.dtype == F32 and src.dtype == F32 and dst.numel() == src.numel() and dst.numel() >= 1
                e.dst, e.src, e.n = _ptr(dst), _ptr(src), dst.numel()
            self.pl.keep.append(arr)
            s.c("mh_accum_spans_f32", arr, len(chunk))

    def site(self, p_, sid) -> Site:
        return Site(self.rng.data_ptr(), float(p_), int(sid)) if p_ > 0 else NO_DROP

    def seg(self, name) -> Segment:
        s = Segment(name, self.eng.lib)
        (self.pl.bwd_add if self.accum else self.pl.bwd).append(s)
        return s

    # ---- packers: typed jobs -> one prepared grouped launch --------------------------------------------------
    def _gemm(self, seg: Segment, probs: List[Gemm], a_k: bool, b_k: bool, lane: int = 0):
        n, pl, T16 = len(probs), self.pl, self.T16
        assert 1 <= n <= _lib.MH_GEMM_MAX_GROUP
        arr = (MhGemmProblem * n)()
        for e, d in zip(arr, probs):
            A, Bm, Cm, M, N, K, lda, ldb, ldc = d[:9]
            assert A.dtype == T16 and Bm.dtype == T16 and Cm.dtype in (T16, F32)
            a_need = (K - 1) * lda + M if a_k else (M - 1) * lda + K
            b_need = (K - 1) * ldb + N if b_k else (N - 1) * ldb + K
            assert A.numel() >= a_need and Bm.numel() >= b_need and Cm.numel() >= (M - 1) * ldc + N, (M, N, K)
            for key, t, dt, need in (("bias", d.bias, F32, N), ("residual", d.residual, T16, (M - 1) * ldc + N),
                                     ("aux", d.aux, T16, (M - 1) * ldc + N), ("mul", d.mul, T16, (M - 1) * ldc + N),
                                     ("rowsum", d.rowsum, F32, M)):
                assert t is None or (t.dtype == dt and t.numel() >= need), key
            e.A, e.B, e.C = _ptr(A), _ptr(Bm), _ptr(Cm)
            e.bias, e.residual, e.aux = _ptr(d.bias), _ptr(d.residual), _ptr(d.aux)
            e.mul, e.rowsum = _ptr(d.mul), _ptr(d.rowsum)
            e.M, e.N, e.K, e.lda, e.ldb, e.ldc = M, N, K, lda, ldb, ldc
            e.flags = (MH_GEMM_GELU if d.gelu else 0) | (MH_GEMM_OUT_F32 if Cm.dtype == F32 else 0) | \
                      (MH_GEMM_QUICK_GELU if d.quick else 0) | (MH_GEMM_DERIV_AUX if d.deriv_aux else 0) | \
                      (MH_GEMM_ACCUM if d.accum else 0)
            assert not d.accum or Cm.dtype == F32
            e.alpha = float(d.alpha)
            if d.drop.rng is not None:
                e.drop_rng, e.drop_p, e.drop_stream = d.drop
                e.drop_rows = _ptr(d.drop_rows)
            e.rows_dev = _ptr(d.rows_dev)
        pl.keep.append(arr)
        fl = [2.0 * d.M * d.N * d.K for d in probs]
        dyn = float(sum(x for x, d in zip(fl, probs) if d.rows_dev is not None))    # scales with the live rows
        fixed = float(sum(fl)) - dyn
        pl.gemm_flops += fixed + dyn
        pl.gemm_flops_dyn += dyn
        seg.c("mh_gemm_bf16_grouped", arr, n, int(a_k), int(b_k), tag=f"gemm<{int(a_k)},{int(b_k)}>", work=(fixed, dyn),
              lane=lane)

    @staticmethod
    def _fwd_prob(x, w, out, T, N, K, **kw) -> Gemm:
        return Gemm(x, w, out, T, N, K, lda=K, ldb=K, ldc=N, **kw)

    @staticmethod
    def _dgrad_prob(dy, w, out, T, N_out, K_in, **kw) -> Gemm:
        # out[T, K_in] = dy[T, N_out] @ w[N_out, K_in]
        return Gemm(dy, w, out, T, K_in, N_out, lda=N_out, ldb=K_in, ldc=K_in, **kw)

    def _wgrad_prob(self, dy, x, dw, db, T, N_out, K_in, **kw) -> Gemm:
        # dw[N_out, K_in] = dy[T, N_out]^T @ x[T, K_in]   (dy carries the gradient-stream scale: alpha removes it)
        return Gemm(dy, x, dw, N_out, K_in, T, lda=N_out, ldb=K_in, ldc=K_in, rowsum=db, alpha=1.0 / self.eng.gscale, **kw)

    # the three GEMMs of one Linear of layer l of a tower (`stem`.weight / `stem`.bias; count = 3: the fused q/k/v)
    def _linear(self, tw: Tower, l, stem, x, out, M, N, K, count=1, **kw) -> Gemm:
        nm = tw.name(l, stem)
        return self._fwd_prob(x, self.eng.w(nm + ".weight", count), out, M, N, K, bias=self.eng.p(nm + ".bias", count), **kw)

    def _linear_dgrad(self, tw: Tower, l, stem, dy, out, M, N_out, K_in, count=1, **kw) -> Gemm:
        return self._dgrad_prob(dy, self.eng.w(tw.name(l, stem) + ".weight", count), out, M, N_out, K_in, **kw)

    def _linear_wgrad(self, tw: Tower, l, stem, dy, x, M, N_out, K_in, count=1, **kw) -> Gemm:
        nm = tw.name(l, stem)
        # adding flavour: the matrix gradient is added to in the epilogue (the old value is read once, there); the bias gradient
        # (`rowsum`, overwritten also under MH_GEMM_ACCUM) goes to the mirror
        return self._wgrad_prob(dy, x, self.g(nm + ".weight", count), self.g(nm + ".bias", count), M, N_out, K_in, accum=self.accum, **kw)

    def _ln_fwd_job(self, x, name, y, mean, rstd, rows, D, eps, y32=None, rows_dev=None) -> LnFwd:
        return LnFwd(x, self.eng.p(name + ".weight"), self.eng.p(name + ".bias"), y, mean, rstd, rows, D, float(eps), y32, rows_dev)

    def _ln_bwd_job(self, dy, x, name, mean, rstd, dx, rows, D, dx_add=None, dx_drop=None, drop=NO_DROP, rows_dev=None,
                    drop_rows=None) -> LnBwd:
        part = self.alloc(f"lnpart.{name}.weight", (2, LN_PARTS, D), F32)
        self.pl._ln_jobs.setdefault(D, []).append((part, self.g(name + ".weight"), self.g(name + ".bias")))
        on = drop.rng is not None and dx_drop is not None
        return LnBwd(dy, x, self.eng.p(name + ".weight"), mean, rstd, dx, part, rows, D, dx_add, dx_drop if on else None,
                     drop if on else NO_DROP, rows_dev, drop_rows if on else None)

    def _ln(self, seg: Segment, jobs: list, fn_name: str, struct, fill):
        """LayerNorms that sit at the same point of the lockstep schedule go out as ONE grouped launch per width."""
        by_d: Dict[int, list] = {}
        for j in jobs:
            if j is not None:
                by_d.setdefault(j.D, []).append(j)
        for D, js in by_d.items():
            assert len(js) <= _lib.MH_LN_MAX_JOBS
            arr = (struct * len(js))()
            for e, j in zip(arr, js):
                fill(e, j)
            self.pl.keep.append(arr)
            seg.c(fn_name, arr, len(js), D)

    def _ln_fwd(self, seg: Segment, jobs: List[Optional[LnFwd]]):
        self._ln(seg, jobs, "mh_layernorm_fwd_grouped", MhLnFwdJob, _fill_ln_fwd)

    def _ln_bwd(self, seg: Segment, jobs: List[Optional[LnBwd]]):
        self._ln(seg, jobs, "mh_layernorm_bwd_grouped", MhLnBwdJob, _fill_ln_bwd)

    def _attn(self, seg: Segment, probs: List[Attn], backward: bool):
        """Both towers' attention of a layer pair as one grouped call (one launch per kernel when the pair fits the
        dual kernels, see include/memehip.h: mh_attn_fwd_grouped)."""
        arr = (MhAttnProblem * len(probs))()
        for e, d in zip(arr, probs):
            for k in ("qkv", "key_mask", "out", "lse", "dout", "delta", "dqkv", "cu", "row_map"):
                setattr(e, k, _ptr(getattr(d, k)))
            e.rng, e.drop_p, e.drop_stream = d.drop
            e.B, e.S, e.H = d.B, d.S, d.H
            n = d.B * d.S * d.H * 64
            assert d.qkv.numel() >= 3 * n and d.out.numel() >= n and d.lse.numel() >= d.B * d.H * d.S
            if backward:
                assert d.dout.numel() >= n and d.dqkv.numel() >= 3 * n and d.delta.numel() >= d.B * d.H * d.S
        self.pl.keep.append(arr)
        seg.c("mh_attn_bwd_grouped" if backward else "mh_attn_fwd_grouped", arr, len(probs))

    def _attn_prob(self, tw: Tower, l: int, **bw) -> Attn:
        a = tw.acts[l]
        return Attn(a.qkv, a.ctx, a.lse, self.B, tw.S, tw.H, tw.key_mask, tw.cu, tw.row_map,
                    self.site(tw.p_a, 16 * (l + 1) + 1), **bw)

    def _rows(self, seg: Segment, jobs: List[RowsJob], scatter: bool):
        """Row jobs of the last layer as ONE launch: gather (full -> compact [n, D]) or scatter with zero fill (compact -> full)."""
        if not jobs:
            return
        assert len(jobs) <= _lib.MH_ROWS_MAX_JOBS
        arr = (MhRowsJob * len(jobs))()
        for e, j in zip(arr, jobs):
            full, compact = (j.dst, j.src) if scatter else (j.src, j.dst)
            assert j.src.dtype == self.T16 and j.dst.dtype == self.T16 and full.numel() >= j.rows * j.D and compact.numel() >= j.n * j.D
            assert j.idx is None or (j.idx.dtype == torch.int32 and j.idx.numel() >= j.n)
            e.src, e.dst, e.idx, e.rows_dev = _ptr(j.src), _ptr(j.dst), _ptr(j.idx), _ptr(j.rows_dev if scatter else None)
            e.n, e.rows, e.D, e.stride, e.offset = j.n, j.rows, j.D, j.stride, j.offset
        self.pl.keep.append(arr)
        seg.c("mh_rows_scatter_zero" if scatter else "mh_rows_gather", arr, len(jobs))

    # ---- forward --------------------------------------------------------------------------------------------------
    def text_embed(self):
        """Text embeddings (dense [B*S] rows: the tables are indexed by position), then the row packing."""
        eng, f, tw, t, B, S, alloc = self.eng, self.pl.fwd, self.text, self.cfg.text, self.B, self.S, self.alloc
        Tt, Dt = tw.T, tw.D
        self.ids, self.mask = alloc("ids", (B, S), I64, zero=True), alloc("mask", (B, S), I64, zero=True)      # static inputs
        self.prev_ids = alloc("prev_ids", (B, S), I64, zero=True)
        self.pre0 = alloc("t.pre0", (Tt, Dt))
        x0d = alloc("t.x0", (Tt, Dt))
        self.m0, self.r0 = alloc("t.m0", (Tt,), F32), alloc("t.r0", (Tt,), F32)
        type0 = eng.p(TXT + "embeddings.token_type_embeddings.weight")[:Dt] if t.type_vocab > 0 else None
        embed = (_ptr(self.ids), _ptr(eng.p(TXT + "embeddings.word_embeddings.weight")),
                 _ptr(eng.p(TXT + "embeddings.position_embeddings.weight")), _ptr(type0),
                 _ptr(eng.p(TXT + "embeddings.LayerNorm.weight")), _ptr(eng.p(TXT + "embeddings.LayerNorm.bias")),
                 _ptr(self.pre0), _ptr(x0d), _ptr(self.m0), _ptr(self.r0), B, S, Dt, t.vocab_size, float(t.ln_eps), *self.site(tw.p_h, 1))
        if t.position_scheme == "roberta":
            # the position rows depend on the batch's ids: computed on the device, inside the (captured) forward.  pos_inv (table
            # row -> position, per sequence) is what the position-table gradient of the local batch reads
            pos_ids = alloc("t.pos_ids", (B, S), torch.int32, zero=True)
            self.pos_inv = alloc("t.pos_inv", (B, t.max_position), torch.int32, zero=True)
            f.c("mh_position_ids_from_input_ids", _ptr(self.ids), _ptr(pos_ids), _ptr(self.pos_inv), B, S, int(t.pad_token_id),
                t.max_position)
            f.c("mh_bert_embed_fwd_pos", *embed, _ptr(pos_ids), t.max_position)
        else:
            f.c("mh_bert_embed_fwd", *embed)
        # padding-free text tower: the encoder layers see only the rows that matter (attention_mask != 0, plus the
        # pooled position), packed back to back.  The row count lives on the device (n_rows): every text launch below
        # is sized for B*S rows and clamps itself at run time, so one plan / one hipGraph serves every batch.
        if self.pl.packed:
            I32 = torch.int32
            cu, row_map = alloc("pk.cu", (B + 1,), I32, zero=True), alloc("pk.row_map", (Tt,), I32, zero=True)
            self.inv_map, pmask = alloc("pk.inv_map", (Tt,), I32, zero=True), alloc("pk.pmask", (Tt,), I64, zero=True)
            self.pool_rows, n_rows = alloc("pk.pool_rows", (B,), I32, zero=True), alloc("pk.n_rows", (1,), I32, zero=True)
            f.c("mh_pack_plan", _ptr(self.mask), B, S, self.pool_index, _ptr(cu), _ptr(row_map), _ptr(self.inv_map), _ptr(pmask),
                _ptr(self.pool_rows), _ptr(n_rows))
            tw.x.append(alloc("t.x0p", (Tt, Dt)))
            f.c("mh_pack_rows", _ptr(x0d), _ptr(row_map), _ptr(n_rows), _ptr(tw.x[0]), Tt, Dt)
            tw.rows_dev, tw.row_map, tw.key_mask, tw.cu = n_rows, row_map, pmask, cu
            # the pooled rows of the tower's row buffers: by the packing plan's pool_rows, or by arithmetic
            tw.pool = RowsJob(B, Tt, Dt, idx=self.pool_rows)
        else:
            self.inv_map = self.pool_rows = None
            tw.x.append(x0d)
            tw.key_mask = self.mask
            tw.pool = RowsJob(B, Tt, Dt, stride=S, offset=self.pool_index)

    def image_embed(self):
        eng, f, tw, v, B, alloc = self.eng, self.pl.fwd, self.image, self.cfg.image, self.B, self.alloc
        Np, Ti, Di = v.n_patches, tw.T, tw.D
        Kp, Kpp = v.patch_dim, v.patch_dim_padded     # contraction of the patch projection (588 -> 640 for CLIP's 14x14 patches)
        image = alloc("image", (B, v.channels, v.image_size, v.image_size), F32, zero=True)      # static input
        self.patches = alloc("i.patches", (B * Np, Kpp))
        proj = alloc("i.proj", (B * Np, Di))
        tw.x.append(alloc("i.x0", (Ti, Di)))
        tw.pool = RowsJob(B, Ti, Di, stride=tw.S, offset=0)
        wp = eng.w(IMG + "embeddings.patch_embeddings.projection.weight")
        if Kpp == Kp and v.patch % 8 == 0:
            f.c("mh_patchify", _ptr(image), _ptr(self.patches), B, v.channels, v.image_size, v.image_size, v.patch)
        else:
            f.c("mh_patchify_ld", _ptr(image), _ptr(self.patches), B, v.channels, v.image_size, v.image_size, v.patch, Kpp)
        if Kpp != Kp:       # zero-padded copy of the [Di][Kp] weight shadow (two 16-bit elements per word)
            wpad = alloc("i.wp_pad", (Di, Kpp))
            f.c("mh_copy2d_u32", _ptr(wp), Kp // 2, _ptr(wpad), Kpp // 2, Di, Kp // 2, Kpp // 2)
            wp = wpad
        pbias = eng.p(IMG + "embeddings.patch_embeddings.projection.bias") if v.patch_bias else None
        self._gemm(f, [self._fwd_prob(self.patches, wp, proj, B * Np, Di, Kpp, bias=pbias)], False, False)
        x0 = alloc("i.x0pre", (Ti, Di)) if v.pre_ln else tw.x[0]
        f.c("mh_vit_assemble_fwd", _ptr(proj), _ptr(eng.p(IMG + "embeddings.cls_token")),
            _ptr(eng.p(IMG + "embeddings.position_embeddings")), _ptr(x0), B, Np, Di)
        if v.pre_ln:        # CLIP: embeddings -> pre_layrnorm -> blocks
            self._ln_fwd(f, [self._ln_fwd_job(x0, IMG + "pre_layernorm", tw.x[0], alloc("i.mpre", (Ti,), F32),
                                              alloc("i.rpre", (Ti,), F32), Ti, Di, v.ln_eps)])

    def last_layer_form(self):
        """The head reads ONE row per sample from each tower (the pooled text position, the ViT class token), and behind the
        attention core every block of a layer is row-wise.  Compact: the last layer of each tower gathers those B rows behind its
        attention and runs out-proj, LayerNorms and FFN on [B, D] panels (forward and backward); the out-proj input
        gradient is scattered back, with zeros everywhere else, in front of the attention backward.  Not when somebody
        reads the full last hidden states ("sequence"), and not with dropout (its masks are indexed by the full row).
        Everything that follows from that choice is set here."""
        pl, B, t, v = self.pl, self.B, self.text, self.image
        cmp = self.last_rows == "pooled" and pl.features != "sequence" and not pl.dropout_on and t.L >= 1 and v.L >= 1
        pl.last_rows = "pooled" if cmp else "all"
        # where the head finds its rows: compact towers hand it [B, D] (one "token" per sample)
        self.head_rows = (1, 1, 0, None) if cmp else (t.S, v.S, self.pool_index, self.pool_rows)     # (S, Nt, pool index, pool rows)
        for tw, n in ((t, "t"), (v, "i")):
            tw.compact = B if cmp else 0
            # the weight-gradient GEMMs of layer l may run on a side stream while the chain of layers l-1 and
            # l-2 proceeds: everything they read is double-buffered by layer parity (dX: rotation of three),
            # and layer l-2 waits for them before it overwrites those buffers
            tw.dX = [self.alloc(f"{n}.dX{i}", (tw.T, tw.D)) for i in range(3)]
            # the gradient that enters each tower's last layer: non-zero at the pooled rows only.  Full rows: zero-filled (bwd_head),
            # the head writes the pooled rows.  Compact: [B, D], every row written by the head.
            tw.d_last = self.alloc(f"{n}.dXrows", (B, tw.D)) if cmp else tw.dX[0]
        self.zero_fill = not cmp

    def layer_buffers(self):
        B, t, v, alloc = self.B, self.text, self.image, self.alloc
        self.xt_last32 = alloc("t.xlast32", (t.out_rows, t.D), F32)   # unrounded tower outputs for the fp32 head
        self.xf32 = alloc("i.xf32", (v.out_rows, v.D), F32)
        for l in range(t.L):
            R, n = t.rows(l), f"t{l}."
            ctx = alloc(n + "ctx", (t.T, t.D))
            t.acts.append(TextActs(
                qkv=alloc(n + "qkv", (t.T, 3 * t.D)), ctx=ctx, lse=alloc(n + "lse", (B, t.H, t.S), F32), a=alloc(n + "a", (R, t.D)),
                y=alloc(n + "y", (R, t.D)), m1=alloc(n + "m1", (R,), F32), r1=alloc(n + "r1", (R,), F32),
                h=alloc(n + "h", (R, t.I)), g=alloc(n + "g", (R, t.I)), f=alloc(n + "f", (R, t.D)),
                m2=alloc(n + "m2", (R,), F32), r2=alloc(n + "r2", (R,), F32),
                pctx=alloc(n + "pctx", (B, t.D)) if R != t.T else ctx, x=alloc(n + "xrows", (B, t.D)) if R != t.T else t.x[l], rows=R))
            t.x.append(alloc(f"t.x{l + 1}", (R, t.D)))
        for l in range(v.L):
            R, n = v.rows(l), f"i{l}."
            ctx = alloc(n + "ctx", (v.T, v.D))
            v.acts.append(ImageActs(
                u=alloc(n + "u", (v.T, v.D)), m1=alloc(n + "m1", (v.T,), F32), r1=alloc(n + "r1", (v.T,), F32),
                qkv=alloc(n + "qkv", (v.T, 3 * v.D)), ctx=ctx, lse=alloc(n + "lse", (B, v.H, v.S), F32),
                xp=alloc(n + "xp", (R, v.D)), w=alloc(n + "w", (R, v.D)), m2=alloc(n + "m2", (R,), F32), r2=alloc(n + "r2", (R,), F32),
                h=alloc(n + "h", (R, v.I)), g=alloc(n + "g", (R, v.I)),
                pctx=alloc(n + "pctx", (B, v.D)) if R != v.T else ctx, x=alloc(n + "xrows", (B, v.D)) if R != v.T else v.x[l], rows=R))
            v.x.append(alloc(f"i.x{l + 1}", (R, v.D)))
        self.xf = alloc("i.xf", (v.out_rows, v.D))
        self.mf, self.rf = alloc("i.mf", (v.out_rows,), F32), alloc("i.rf", (v.out_rows,), F32)
        # the LayerNorm that opens image layer 0 (every later one shares a launch with the text LayerNorm closing the layer above)
        self._ln_fwd(self.pl.fwd, [self._img_ln1(0)])

    def _img_ln1(self, l) -> Optional[LnFwd]:
        """The ViT block's pre-attention LayerNorm of layer l; past the last layer, the final ViT LayerNorm.
        It is issued together with the text tower's LayerNorm that closes layer l-1 (one grouped launch)."""
        v = self.image
        if l < v.L:
            b = v.acts[l]
            return self._ln_fwd_job(v.x[l], v.name(l, "layernorm_before"), b.u, b.m1, b.r1, v.T, v.D, v.eps)
        if l == v.L:
            return self._ln_fwd_job(v.x[l], IMG + "layernorm", self.xf, self.mf, self.rf, v.out_rows, v.D, v.eps, y32=self.xf32)
        return None

    def fwd_layer(self, l):
        """Layer l of both towers in lockstep: every GEMM stage is one grouped launch over the towers that have a layer l."""
        f, t, v = self.pl.fwd, self.text, self.image
        lay = [(tw, tw.acts[l], tw.roles(l), tw.rows(l)) for tw in self.towers if l < tw.L]
        a, b = (t.acts[l] if l < t.L else None), (v.acts[l] if l < v.L else None)
        # QKV
        self._gemm(f, [self._linear(tw, l, tw.attn + "query", r.attn_in, a_.qkv, tw.T, 3 * tw.D, tw.D, 3, **tw.live(tw.T))
                       for tw, a_, r, M in lay], False, False)
        self._attn(f, [self._attn_prob(tw, l) for tw, _, _, _ in reversed(lay)], backward=False)
        # a compact last layer: from here on, only the pooled rows (of the attention output and of the layer input)
        self._rows(f, [j for tw, a_, r, M in lay if M != tw.T
                       for j in (tw.pool._replace(src=a_.ctx, dst=a_.pctx), tw.pool._replace(src=tw.x[l], dst=a_.x))], scatter=False)
        # attention output projection + residual
        self._gemm(f, [self._linear(tw, l, "attention.output.dense", a_.pctx, r.proj_out, M, tw.D, tw.D, residual=a_.x,
                                    drop=self.site(tw.p_h, 16 * (l + 1) + 2), **tw.live(M, drop=True)) for tw, a_, r, M in lay], False, False)
        self._ln_fwd(f, [
            self._ln_fwd_job(a.a, t.name(l, t.ln_mid), a.y, a.m1, a.r1, a.rows, t.D, t.eps, **t.live(a.rows)) if a else None,
            self._ln_fwd_job(b.xp, v.name(l, v.ln_mid), b.w, b.m2, b.r2, b.rows, v.D, v.eps) if b else None])
        # FFN up + GELU; "h" keeps gelu'(pre-activation) for the backward (computed here from the activation's own exponential:
        # MH_GEMM_DERIV_AUX)
        self._gemm(f, [self._linear(tw, l, "intermediate.dense", r.ffn_in, a_.g, M, tw.I, tw.D, aux=a_.h, gelu=True, deriv_aux=True,
                                    quick=tw.quick, **tw.live(M)) for tw, a_, r, M in lay], False, False)
        # FFN down + residual
        self._gemm(f, [self._linear(tw, l, "output.dense", a_.g, r.ffn_out, M, tw.D, tw.I, residual=r.ffn_res,
                                    drop=self.site(tw.p_h, 16 * (l + 1) + 3), **tw.live(M, drop=True)) for tw, a_, r, M in lay], False, False)
        # the text LayerNorm closing this layer + the image LayerNorm opening the next (or the final ViT one)
        self._ln_fwd(f, [
            self._ln_fwd_job(a.f, t.name(l, "output.LayerNorm"), t.x[l + 1], a.m2, a.r2, a.rows, t.D, t.eps,
                             y32=self.xt_last32 if l == t.L - 1 else None, **t.live(a.rows)) if a else None,
            self._img_ln1(l + 1) if b else None])

    def head_and_loss(self):
        eng, pl, f, B, alloc, t, v = self.eng, self.pl, self.pl.fwd, self.B, self.alloc, self.text, self.image
        P_, Cn = self.cfg.proj, self.cfg.num_classes
        self.hp, self.hg = MhHeadParams(), MhHeadGrads()
        for fld, nm in HEAD_FIELDS:
            setattr(self.hp, fld, _ptr(eng.p(nm)))
            setattr(self.hg, fld, _ptr(eng.g(nm)))
        pl.keep += [self.hp, self.hg]
        self.pooled = alloc("h.pooled", (B, t.D + v.D), F32)
        self.feat, self.fused = alloc("h.feat", (B, 2 * P_), F32), alloc("h.fused", (B, P_), F32)
        logits = alloc("logits", (B, Cn), F32)
        S_h, Nt_h, pool_h, rows_h = self.head_rows
        if pl.features == "sequence":
            assert not pl.packed
            self.d_seq_t, self.d_seq_i = alloc("h.d_seq_t", (t.T, t.D), F32, zero=True), alloc("h.d_seq_i", (v.T, v.D), F32, zero=True)
        elif pl.features:
            self.d_pooled = alloc("h.d_pooled", (B, t.D + v.D), F32, zero=True)
            f.c("mh_pool_fwd", _ptr(self.xt_last32), _ptr(self.xf32), pool_h, _ptr(self.pooled), B, S_h, Nt_h, t.D, v.D, _ptr(rows_h))
        else:
            f.c("mh_head_fwd", C.byref(self.hp), _ptr(self.xt_last32), _ptr(self.xf32), pool_h, _ptr(self.pooled), _ptr(self.feat),
                _ptr(self.fused), _ptr(logits), B, S_h, Nt_h, t.D, v.D, P_, Cn, *self.site(self.p_head, 7), _ptr(rows_h))
        labels, loss = alloc("labels", (B,), I64, zero=True), alloc("loss", (1,), F32, zero=True)
        self.dlogits = alloc("dlogits", (B, Cn), F32, zero=True)
        ncorrect = alloc("ncorrect", (1,), torch.int32, zero=True)
        opts = None if pl.features else eng.loss_opts      # (a features plan never runs its loss segment)
        pl.loss_opts = opts
        if opts is None:
            pl.loss.c("mh_ce_fwd_bwd", _ptr(logits), _ptr(labels), _ptr(loss), _ptr(self.dlogits), _ptr(ncorrect), B, Cn,
                      1.0, _ptr(eng.loss_scale))
        else:
            assert not opts.weighted or (eng.class_weight is not None and eng.class_weight.numel() == Cn)
            pl.loss.c("mh_ce_opts_fwd_bwd", _ptr(logits), _ptr(labels), _ptr(eng.class_weight) if opts.weighted else None, _ptr(loss),
                      _ptr(self.dlogits), _ptr(ncorrect), B, Cn, opts.ignore_index or 0, int(opts.ignore_index is not None),
                      opts.label_smoothing, _lib.MH_LOSS_SUM if opts.reduction == "sum" else _lib.MH_LOSS_MEAN, 1.0, _ptr(eng.loss_scale))

    # ---- backward -------------------------------------------------------------------------------------------------
    def bwd_head(self):
        eng, pl, B, alloc, t, v = self.eng, self.pl, self.B, self.alloc, self.text, self.image
        P_, Cn = self.cfg.proj, self.cfg.num_classes
        s = self.seg("bwd_head")
        dXf = alloc("i.dXf", (v.out_rows, v.D))
        dfeat, dfused = alloc("h.dfeat", (B, 2 * P_), F32), alloc("h.dfused", (B, P_), F32)
        S_h, Nt_h, pool_h, rows_h = self.head_rows
        if self.zero_fill:
            s.py(t.d_last.zero_)
            s.py(dXf.zero_)
        if pl.features:
            # the built-in head is not part of this graph: its gradient slots must not keep stale values
            h0 = eng.layout.spec["bert_fc.weight"].offset
            h1 = eng.layout.spec["output_fc.bias"].offset + eng.layout.spec["output_fc.bias"].numel
            if self.accum:      # adding flavour: zeros in the mirror, added like every other small gradient
                head_grads = eng.mirror()[h0 - eng.small0:h1 - eng.small0]
                self.acc_spans.append((h0, h1 - h0))
            else:
                head_grads = eng.G[h0:h1]
            s.py(head_grads.zero_)
            if pl.features == "sequence":      # the caller's gradient w.r.t. every hidden state (already times the stream scale)
                s.c("mh_cast_f32_bf16", _ptr(self.d_seq_t), _ptr(t.d_last), t.T * t.D)
                s.c("mh_cast_f32_bf16", _ptr(self.d_seq_i), _ptr(dXf), v.T * v.D)
            else:
                s.c("mh_pool_bwd", _ptr(self.d_pooled), _ptr(t.d_last), _ptr(dXf), pool_h, B, S_h, Nt_h, t.D, v.D, float(eng.gscale),
                    _ptr(rows_h))
        else:
            hg = self.hg
            if self.accum:
                hg = MhHeadGrads()
                for fld, nm in HEAD_FIELDS:
                    setattr(hg, fld, _ptr(self.g(nm)))
                pl.keep.append(hg)
            s.c("mh_head_bwd", C.byref(self.hp), C.byref(hg), _ptr(self.dlogits), _ptr(self.pooled), _ptr(self.feat),
                _ptr(self.fused), _ptr(dfeat), _ptr(dfused), _ptr(t.d_last), _ptr(dXf), pool_h, B, S_h, Nt_h, t.D, v.D, P_, Cn,
                float(eng.gscale), *self.site(self.p_head, 7), _ptr(rows_h))
        t.grads, v.grads = self._text_grads(), self._image_grads()
        self.t_dpre = alloc("t.dpre", (t.T, t.D))
        self._ln_bwd(s, [
            self._ln_bwd_job(dXf, v.x[v.L], IMG + "layernorm", self.mf, self.rf, v.d_last, v.out_rows, v.D),
            self._text_ln2_bwd(t.L - 1) if t.L >= v.L else None])

    def _text_grads(self) -> List[Grads]:
        """The gradient buffers of every text layer."""
        t, B, alloc = self.text, self.B, self.alloc
        # backward temporaries, one set per layer parity
        dh = [alloc(f"t.dh{i}", (t.T, t.I)) for i in range(2)]
        da = [alloc(f"t.da{i}", (t.T, t.D)) for i in range(2)]
        dqkv = [alloc(f"t.dqkv{i}", (t.T, 3 * t.D)) for i in range(2)]
        # da times the dropout mask of the Linear output that fed the LayerNorm = gradient w.r.t. the (dropped) attention output
        # dense; without dropout, da itself
        dam = [alloc(f"t.dam{i}", (t.T, t.D)) for i in range(2)] if t.p_h > 0 else da
        # df (gradient at the FFN output) is written one segment EARLY, by the LayerNorm backward grouped into the
        # end of the layer above: rotation of three, so the side-stream GEMMs of layer l+1 never see it overwritten
        df = [alloc(f"t.df{i}", (t.T, t.D)) for i in range(3)]
        dfm = [alloc(f"t.dfm{i}", (t.T, t.D)) for i in range(3)] if t.p_h > 0 else df     # w.r.t. the (dropped) FFN output dense
        dy, dctx = alloc("t.dy", (t.T, t.D)), alloc("t.dctx", (t.T, t.D))
        t.delta = alloc("t.delta", (B, t.H, t.S), F32)
        out = [Grads(d_out=dfm[l % 3], dh=dh[l & 1], d_mid=dy, d_proj=dam[l & 1], res=da[l & 1], dctx=dctx, res_full=da[l & 1],
                     dctx_full=dctx, dqkv=dqkv[l & 1], d_in=t.d_x(l - 1), df=df[l % 3]) for l in range(t.L)]
        if t.compact:
            # the compact last layer's own gradient panels.  The two that reach past the attention output projection are
            # scattered into the full buffers of that layer parity, which the full-size kernels then read as before.
            c_df, c_dh, c_dy = alloc("t.dfrows", (B, t.D)), alloc("t.dhrows", (B, t.I)), alloc("t.dyrows", (B, t.D))
            c_da, c_dctx = alloc("t.darows", (B, t.D)), alloc("t.dctxrows", (B, t.D))
            if t.rows(t.L - 1) != t.T:
                out[-1] = out[-1]._replace(d_out=c_df, dh=c_dh, d_mid=c_dy, d_proj=c_da, res=c_da, dctx=c_dctx, df=c_df)
        return out

    def _image_grads(self) -> List[Grads]:
        v, B, alloc = self.image, self.B, self.alloc
        dh = [alloc(f"i.dh{i}", (v.T, v.I)) for i in range(2)]
        dxp = [alloc(f"i.dxp{i}", (v.T, v.D)) for i in range(2)]
        dqkv = [alloc(f"i.dqkv{i}", (v.T, 3 * v.D)) for i in range(2)]
        dw, dctx, du = alloc("i.dw", (v.T, v.D)), alloc("i.dctx", (v.T, v.D)), alloc("i.du", (v.T, v.D))
        v.delta = alloc("i.delta", (B, v.H, v.S), F32)
        out = [Grads(d_out=v.d_x(l), dh=dh[l & 1], d_mid=dw, d_proj=dxp[l & 1], res=dxp[l & 1], dctx=dctx, res_full=dxp[l & 1],
                     dctx_full=dctx, dqkv=dqkv[l & 1], d_in=du) for l in range(v.L)]
        if v.compact:
            c_dh, c_dw = alloc("i.dhrows", (B, v.I)), alloc("i.dwrows", (B, v.D))
            c_dxp, c_dctx = alloc("i.dxprows", (B, v.D)), alloc("i.dctxrows", (B, v.D))
            if v.rows(v.L - 1) != v.T:
                out[-1] = out[-1]._replace(dh=c_dh, d_mid=c_dw, d_proj=c_dxp, res=c_dxp, dctx=c_dctx)
        return out

    def _text_ln2_bwd(self, l) -> Optional[LnBwd]:
        """Backward of the LayerNorm that closes text layer l.  Issued at the END of the segment above, grouped with the
        image tower's LayerNorm there."""
        t = self.text
        if not (0 <= l < t.L):
            return None
        a, g = t.acts[l], t.grads[l]
        return self._ln_bwd_job(t.d_x(l), a.f, t.name(l, "output.LayerNorm"), a.m2, a.r2, g.df, a.rows, t.D, dx_drop=g.d_out,
                                drop=self.site(t.p_h, 16 * (l + 1) + 3), **t.live(a.rows, drop=True))

    def _text_embed_ln_bwd(self, s: Segment) -> LnBwd:
        """Backward of the text embedding LayerNorm, with what has to run in front of it."""
        t = self.text
        d_emb = t.d_x(-1)
        if self.pl.packed:        # back to dense [B*S] rows (zeros at the dropped positions) for the embedding tables
            d_emb = self.alloc("t.dX_dense", (t.T, t.D))
            s.c("mh_unpack_rows", _ptr(t.d_x(-1)), _ptr(self.inv_map), _ptr(d_emb), t.T, t.D)
        if t.p_h > 0:     # gradient w.r.t. the dropped embedding output -> w.r.t. the LayerNorm output
            s.c("mh_dropout_apply", _ptr(d_emb), t.T * t.D, self.rng.data_ptr(), float(t.p_h), 1)
        return self._ln_bwd_job(d_emb, self.pre0, TXT + "embeddings.LayerNorm", self.m0, self.r0, self.t_dpre, t.T, t.D)

    def bwd_layer(self, l):
        """Backward of layer l of both towers.  The GEMM stages are stated once; where the dataflow differs -- the post-LN text
        tower adds its residual gradients as the `residual` of a dgrad GEMM, the pre-LN image tower as `dx_add` of a LayerNorm
        backward -- the two towers have a job each."""
        t, v = self.text, self.image
        s = self.seg(f"bwd_layer_{l}")
        s.wait(f"bwd_layer_{l + 2}")
        lay = [(tw, tw.acts[l], tw.roles(l), tw.grads[l], tw.rows(l)) for tw in self.towers if l < tw.L]
        a, ga = (t.acts[l], t.grads[l]) if l < t.L else (None, None)
        b, gb = (v.acts[l], v.grads[l]) if l < v.L else (None, None)
        # d gelu_in = (d_out @ W2) * gelu'(h)
        self._gemm(s, [self._linear_dgrad(tw, l, "output.dense", g.d_out, g.dh, M, tw.D, tw.I, mul=a_.h, deriv_aux=True, quick=tw.quick,
                                          **tw.live(M)) for tw, a_, r, g, M in lay], False, True)
        # through W1 (text adds the residual branch df)
        self._gemm(s, [self._linear_dgrad(tw, l, "intermediate.dense", g.dh, g.d_mid, M, tw.I, tw.D, residual=g.df, **tw.live(M))
                       for tw, a_, r, g, M in lay], False, True)
        self._ln_bwd(s, [
            self._ln_bwd_job(ga.d_mid, a.a, t.name(l, t.ln_mid), a.m1, a.r1, ga.res, a.rows, t.D, dx_drop=ga.d_proj,
                             drop=self.site(t.p_h, 16 * (l + 1) + 2), **t.live(a.rows, drop=True)) if a else None,
            self._ln_bwd_job(gb.d_mid, b.xp, v.name(l, v.ln_mid), b.m2, b.r2, gb.res, b.rows, v.D, dx_add=gb.d_out) if b else None])
        # through the attention output projection
        self._gemm(s, [self._linear_dgrad(tw, l, "attention.output.dense", g.d_proj, g.dctx, M, tw.D, tw.D, **tw.live(M))
                       for tw, a_, r, g, M in lay], False, True)
        # a compact last layer ends here: its gradient w.r.t. the attention output goes back to the pooled rows of the full
        # buffer, zeros everywhere else (no row attends for the loss but the pooled one), and the attention backward runs
        # as ever.  The same for the residual branch around the attention (text: da, the `residual` of the QKV dgrad; image:
        # dxp, the `dx_add` of the LayerNorm backward that opens the layer): those kernels add a full buffer, so they get one
        # that is zero off the pooled rows -- adding the panel behind them instead would round twice.
        self._rows(s, [j for tw, a_, r, g, M in lay if M != tw.T
                       for j in (tw.pool._replace(src=g.dctx, dst=g.dctx_full, rows_dev=tw.rows_dev),
                                 tw.pool._replace(src=g.res, dst=g.res_full, rows_dev=tw.rows_dev))], scatter=True)
        self._attn(s, [self._attn_prob(tw, l, dout=g.dctx_full, delta=tw.delta, dqkv=g.dqkv) for tw, a_, r, g, M in reversed(lay)],
                   backward=True)
        # through the QKV projection (text adds the residual branch da)
        self._gemm(s, [self._linear_dgrad(tw, l, tw.attn + "query", g.dqkv, g.d_in, tw.T, 3 * tw.D, tw.D, 3,
                                          residual=g.res_full if tw.post_ln else None, **tw.live(tw.T)) for tw, a_, r, g, M in lay], False, True)
        # the image LayerNorm that opens this layer + the text LayerNorm that closes the layer below (at layer 0:
        # the text embedding LayerNorm), one grouped launch
        t_job = self._text_ln2_bwd(l - 1) if l >= 1 else self._text_embed_ln_bwd(s)
        self._ln_bwd(s, [
            t_job,
            self._ln_bwd_job(gb.d_in, v.x[l], v.name(l, "layernorm_before"), b.m1, b.r1, v.d_x(l - 1), v.T, v.D,
                             dx_add=gb.res_full) if b else None])
        # weight gradients (+ bias gradients as row sums): one grouped launch per tower.  The 4+4 problems in ONE launch (864 tiles)
        # measured 254 us against 215 us for the two 432-tile launches back to back (round 1), and in the step 11.2 ms against 10.2 ms
        # (round 3, with or without a tile order giving every XCD its share of every problem, tools/lab/RESULTS.md (r3k)): the side stream must not hold every workgroup
        # slot -- two 432-tile launches leave 80 of the 512 slots to the main chain.
        for tw, a_, r, g, M in lay:
            self._gemm(s, [
                self._linear_wgrad(tw, l, "output.dense", g.d_out, a_.g, M, tw.D, tw.I, **tw.live(M)),
                self._linear_wgrad(tw, l, "intermediate.dense", g.dh, r.ffn_in, M, tw.I, tw.D, **tw.live(M)),
                self._linear_wgrad(tw, l, "attention.output.dense", g.d_proj, a_.pctx, M, tw.D, tw.D, **tw.live(M)),
                self._linear_wgrad(tw, l, tw.attn + "query", g.dqkv, r.attn_in, tw.T, 3 * tw.D, tw.D, 3, **tw.live(tw.T))],
                True, True, lane=1)
        rng = [r for r in self.eng.layout.layer_ranges if r[0] == l][0]
        self.pl.bucket_after[s.name] = (rng[1], rng[2])

    def bwd_embed(self):
        eng, pl, B, alloc, v, tw = self.eng, self.pl, self.B, self.alloc, self.cfg.image, self.image
        Np, Ti, Di = v.n_patches, tw.T, tw.D
        s = self.seg("bwd_embed")
        i_dproj = alloc("i.dproj", (B * Np, Di))
        d_x0 = tw.d_x(-1)
        if v.pre_ln:        # through CLIP's pre_layrnorm
            d_x0 = alloc("i.dx0pre", (Ti, Di))
            self._ln_bwd(s, [self._ln_bwd_job(tw.d_x(-1), pl.buf["i.x0pre"], IMG + "pre_layernorm", pl.buf["i.mpre"], pl.buf["i.rpre"],
                                              d_x0, Ti, Di)])
        s.c("mh_vit_assemble_bwd", _ptr(d_x0), _ptr(i_dproj), _ptr(self.g(IMG + "embeddings.cls_token")),
            _ptr(self.g(IMG + "embeddings.position_embeddings")), B, Np, Di, 1.0 / eng.gscale)
        self._patch_wgrad(s, i_dproj)
        if self.gather_world <= 0:
            self._table_grads(s, self.ids, self.t_dpre, self.prev_ids, B)
        # finish every LayerNorm's dgamma / dbeta from the partials
        for D, jobs in pl._ln_jobs.items():
            for i0 in range(0, len(jobs), _lib.MH_COLSUM_MAX_JOBS):
                chunk = jobs[i0:i0 + _lib.MH_COLSUM_MAX_JOBS]
                arr = (MhColsumJob * len(chunk))()
                for j, (part, o0, o1) in enumerate(chunk):
                    arr[j].part, arr[j].out0, arr[j].out1 = _ptr(part), _ptr(o0), _ptr(o1)
                pl.keep.append(arr)
                s.c("mh_colsum_partials_f32", arr, len(chunk), LN_PARTS, D, 1.0 / eng.gscale)
        if self.accum:
            self._accum_spans(s)
        tail0 = eng.layout.layer_ranges[-1][2]
        if self.gather_world <= 0:
            pl.bucket_after[s.name] = (tail0, eng.layout.n_total)
        else:
            self._bwd_embed_tables(s, tail0)

    def _patch_wgrad(self, s: Segment, i_dproj):
        """Weight (and bias) gradient of the patch projection.
        (it is a 36-tile GEMM with a 6272-deep contraction, 115 us on 14 % of the CUs; moving it to the side stream beside the
        table gradients measured 0.12 ms SLOWER per step: it delays the join in front of the optimizer tail)"""
        eng, pl, alloc, v, Di = self.eng, self.pl, self.alloc, self.cfg.image, self.image.D
        Kp, Kpp, Tp = v.patch_dim, v.patch_dim_padded, self.B * v.n_patches
        gw = gw_out = eng.g(IMG + "embeddings.patch_embeddings.projection.weight")
        gb = self.g(IMG + "embeddings.patch_embeddings.projection.bias") if v.patch_bias else None
        nsplit = min(_lib.MH_GEMM_MAX_GROUP, max(1, Tp // 512))
        # adding flavour: the plain case adds in the GEMM epilogue; split-K and padded-K finish through mh_colsum_partials_f32 /
        # mh_copy2d_u32, which overwrite: they finish into a scratch of the weight's size, added at the end of the backward
        plain_add = self.accum and nsplit == 1 and Kpp == Kp
        if self.accum and not plain_add:
            gw = gw_out = alloc("i.dwp_acc", (Di * Kp,), F32)
            self.acc_extra.append((eng.g(IMG + "embeddings.patch_embeddings.projection.weight"), gw_out))
        if Kpp != Kp:       # the GEMM writes a [Di][Kpp] gradient; its first Kp columns are copied into the flat buffer
            gw = alloc("i.dwp_pad", (Di * Kpp,), F32)
        if nsplit > 1:
            # split-K: the contraction over B*Np patches is cut into `nsplit` grouped problems with their own f32
            # outputs (288 tiles instead of 36), summed in a fixed order by the partial-sum kernel
            chunk = -(-Tp // nsplit)
            chunk = -(-chunk // 8) * 8
            part_w = alloc("i.dwp_part", (2, nsplit, Di * Kpp), F32)      # [which][split][Di*Kpp]; which = 1 unused
            part_b = alloc("i.dbp_part", (2, nsplit, Di), F32)
            probs = []
            for i in range(nsplit):
                k0 = i * chunk
                kk = min(chunk, Tp - k0)
                if kk <= 0:
                    part_w[0, i].zero_(), part_b[0, i].zero_()
                    continue
                probs.append(self._wgrad_prob(i_dproj[k0:], self.patches[k0:], part_w[0, i], part_b[0, i], kk, Di, Kpp))
            self._gemm(s, probs, True, True)
            for part, out, D_ in ((part_w, gw, Di * Kpp), (part_b, gb, Di)):
                if out is None:
                    continue
                arr = (MhColsumJob * 1)()
                arr[0].part, arr[0].out0, arr[0].out1 = _ptr(part), _ptr(out), None
                pl.keep.append(arr)
                s.c("mh_colsum_partials_f32", arr, 1, nsplit, D_, 1.0)
        else:
            self._gemm(s, [self._wgrad_prob(i_dproj, self.patches, gw, gb, Tp, Di, Kpp, accum=plain_add)], True, True)
        if Kpp != Kp:
            s.c("mh_copy2d_u32", _ptr(gw), Kpp, _ptr(gw_out), Kp, Di, Kp, Kp)

    def _table_grads(self, sg: Segment, ids_, dpre_, prev_, nb):
        eng, t, S, Dt = self.eng, self.cfg.text, self.S, self.text.D
        roberta = t.position_scheme == "roberta"
        gword = eng.g(WORD_TABLE)
        # (only row 0 of the token-type table and, in the bert scheme, the first S rows of the position table are written)
        gtype0 = self.g(TXT + "embeddings.token_type_embeddings.weight", written=Dt)[:Dt] if t.type_vocab > 0 else None
        gpos = self.g(TXT + "embeddings.position_embeddings.weight", written=None if roberta else S * Dt)
        # dense-Adam semantics: the table gradient is dense; only rows touched last step need re-zeroing.  The adding flavour
        # clears nothing: it adds its row sums to the rows it touches (untouched rows are zero) and leaves its ids with the engine,
        # for the first backward of the next window (Engine.before_backward)
        if not self.accum:
            sg.c("mh_zero_rows_f32", _ptr(prev_), _ptr(gword), nb * S, Dt, t.vocab_size)
        # roberta scheme: the per-position sums of mh_bert_embed_bwd (which the token-type gradient is made of) go to a scratch,
        # and the position table gets its gradient by table row below
        dpos = self.alloc("t.dpos_by_s", (S, Dt), F32) if roberta else gpos
        sg.c("mh_bert_embed_bwd_accum" if self.accum else "mh_bert_embed_bwd", _ptr(ids_), _ptr(dpre_), _ptr(gword), _ptr(dpos), _ptr(gtype0),
             nb, S, Dt, t.vocab_size, int(t.pad_token_id), 1.0 / eng.gscale, eng.word_row_live.data_ptr(), eng.word_first.data_ptr(),
             eng.word_count.data_ptr())
        if roberta:
            pos_inv = self.pos_inv
            if ids_ is not self.ids:       # the gathered sequences of every rank: their own position ids
                pos_ids = self.alloc("t.pos_ids_all", (nb, S), torch.int32, zero=True)
                pos_inv = self.alloc("t.pos_inv_all", (nb, t.max_position), torch.int32, zero=True)
                sg.c("mh_position_ids_from_input_ids", _ptr(ids_), _ptr(pos_ids), _ptr(pos_inv), nb, S, int(t.pad_token_id),
                     t.max_position)
            # writes every row of the table gradient (zeros where no token reads the row): nothing to re-zero
            sg.c("mh_embed_pos_bwd", _ptr(dpre_), _ptr(pos_inv), _ptr(gpos), None, None, nb, S, Dt, t.max_position,
                 1.0 / eng.gscale)
        if self.accum:
            window = eng._window_ids       # (the list, not the engine: a callback that held the engine would tie plan and engine into a cycle)
            sg.py(lambda: window.append(ids_.clone()))
        else:
            sg.py(lambda: prev_.copy_(ids_))

    def _bwd_embed_tables(self, s: Segment, tail0: int):
        """Data parallel: word / position / token-type tables sit at the end of the flat buffer; their gradients
        come from the gathered rows of every rank (already the global sum), so the all-reduce stops before them."""
        eng, pl, t, B, S, W, alloc = self.eng, self.pl, self.cfg.text, self.B, self.S, self.gather_world, self.alloc
        Tt, Dt = self.text.T, self.text.D
        first_tbl = TXT + ("embeddings.token_type_embeddings.weight" if t.type_vocab > 0
                           else "embeddings.position_embeddings.weight")
        tbl0 = eng.layout.spec[first_tbl].offset
        assert eng.layout.spec[TXT + "embeddings.word_embeddings.weight"].offset + t.vocab_size * Dt + 3 >= eng.layout.n_total - 3
        pl.bucket_after[s.name] = (tail0, tbl0)
        ids_all = alloc("ids_all", (W * B, S), I64, zero=True)
        prev_all = alloc("prev_ids_all", (W * B, S), I64, zero=True)
        dpre_all = alloc("t.dpre_all", (W * Tt, Dt))
        pl.gather = [(self.ids, ids_all), (self.t_dpre, dpre_all)]      # (local, gathered) pairs, exchanged between segments
        self._table_grads(self.seg("bwd_embed_tables"), ids_all, dpre_all, prev_all, W * B)
