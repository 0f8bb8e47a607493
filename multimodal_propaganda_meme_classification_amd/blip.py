"""BLIP image captioning (``BlipForConditionalGeneration.generate``: greedy, beam search or sampling) on the HIP kernels: the caption tower of Kevin's model.

The reference captions every image of every split inside ``MultimodalDataset.__init__`` (``Multimodal_example_task2C.py:195-256``):
``Salesforce/blip-image-captioning-large`` in fp16, the prompt ``"a meme of"``, batches of 64, ``generate(..., max_new_tokens=128)``.
``BlipCaptioner`` holds that model's parameters under transformers' state_dict names (``vision_model.*``, ``text_decoder.bert.*``,
``text_decoder.cls.predictions.*``), so its checkpoint loads ``strict=True``, and ``generate`` returns the same token ids.

Launch plan (activations are 16-bit row matrices, ``compute_dtype`` selects the bf16 or the fp16 library):

* vision tower, forward only: ``mh_patchify`` + the patch GEMM, ``mh_vit_assemble_fwd`` (class token + positions), per pre-LN layer
  LayerNorm -> QKV GEMM -> ``mh_attn_fwd`` -> projection GEMM (+ residual) -> LayerNorm -> fc1 (erf-GELU) -> fc2 (+ residual); then
  ``post_layernorm``;
* every decoder layer's cross-attention k / v over the image rows: grouped GEMMs, once per batch, into ``[B][577][k | v]``;
* the decode step, one token per row: ``mh_decode_embed`` (word[id] + pos[t], LayerNorm); per layer the packed QKV GEMM,
  ``mh_attn_decode`` (self: stores this step's k / v into cache slot t, attends 0..t), out-proj + residual, LayerNorm, cross Q GEMM,
  ``mh_attn_decode`` (cross, 577 keys), out-proj + residual, LayerNorm, FFN (GELU epilogue), FFN + residual, LayerNorm; then the
  LM-head transform (GEMM + GELU, LayerNorm), the decoder GEMM into f32 logits (vocabulary padded to a multiple of 128 with zero
  rows) and ``mh_greedy_step``.  The prompt goes through the same step one token at a time (causal: the same result as a prefill).
* The step reads t, the input ids and the finished flags on the device, so it is captured once as a single-stream hipGraph and
  replayed per token; the host reads the "all rows finished" word every ``poll_every`` steps.
* Beam search (``num_beams = K > 1``) runs the same step on B * K rows, [image][beam]: ``mh_beam_step`` replaces ``mh_greedy_step``
  (transformers' ``_beam_search``: top 2K of the K * V accumulated log-probabilities, running and finished beams, the early-stop
  heuristic, all on the device), cross-attention reads one k / v copy per image (``kv_group = K``), and the self-attention cache
  stays in place: an int32 ancestry table [B * K][cap], permuted by ``mh_beam_step``, tells ``mh_attn_decode`` which physical row
  holds each earlier position of a beam.
* Logits processors (``repetition_penalty``, ``no_repeat_ngram_size``, ``min_length``, ``min_new_tokens``) run inside the two
  selection kernels (``mh_greedy_step_processed`` / ``mh_beam_step_processed``): the row's history is staged into LDS and turned
  into two bitmaps over the vocabulary, which the kernels' existing passes over the logits look up.  The settings are baked into
  the captured step (the minimum lengths are compared with the device step counter), so other settings re-capture it.
* Sampling (``do_sample=True``) replaces ``mh_greedy_step`` by ``mh_sample_step``: processors, temperature, top-k and top-p as
  transformers orders them, then one multinomial draw per row, all in one workgroup per row and in fixed-order sums.  The draw's
  uniform is a counter hash of (seed, row, column); the seed lives in device memory, so the captured step serves every seed, while
  the temperature, top-k and top-p are baked in.  ``num_return_sequences = n`` runs B * n rows, [image][k], over one copy of each
  image's cross-attention k / v (``kv_group = n``).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import _lib, ops

F32, I32, I64 = torch.float32, torch.int32, torch.int64

_TEXT_DEFAULTS = dict(vocab_size=30524, hidden_size=768, encoder_hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                      num_attention_heads=8, max_position_embeddings=512, layer_norm_eps=1e-12, hidden_act="gelu",
                      bos_token_id=30522, pad_token_id=0, sep_token_id=102)
_VISION_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, image_size=384,
                        patch_size=16, layer_norm_eps=1e-5, hidden_act="gelu", num_channels=3)


def _section(cfg, name, defaults):
    sub = cfg.get(name) if isinstance(cfg, dict) else getattr(cfg, name)
    if sub is None:
        sub = {}
    if not isinstance(sub, dict):
        sub = sub.to_dict()
    return {k: sub.get(k, v) for k, v in defaults.items()}


def _lin(i, o):
    return nn.Linear(i, o)


class _VisionLayer(nn.Module):
    def __init__(self, D, I, eps):
        super().__init__()
        self.self_attn = nn.Module()
        self.self_attn.qkv = _lin(D, 3 * D)
        self.self_attn.projection = _lin(D, D)
        self.layer_norm1 = nn.LayerNorm(D, eps=eps)
        self.mlp = nn.Module()
        self.mlp.fc1 = _lin(D, I)
        self.mlp.fc2 = _lin(I, D)
        self.layer_norm2 = nn.LayerNorm(D, eps=eps)


class _TextAttention(nn.Module):
    def __init__(self, D, Dkv, eps):
        super().__init__()
        self.self = nn.Module()
        self.self.query = _lin(D, D)
        self.self.key = _lin(Dkv, D)
        self.self.value = _lin(Dkv, D)
        self.output = nn.Module()
        self.output.dense = _lin(D, D)
        self.output.LayerNorm = nn.LayerNorm(D, eps=eps)


class _TextLayer(nn.Module):
    def __init__(self, D, Denc, I, eps):
        super().__init__()
        self.attention = _TextAttention(D, D, eps)
        self.crossattention = _TextAttention(D, Denc, eps)
        self.intermediate = nn.Module()
        self.intermediate.dense = _lin(D, I)
        self.output = nn.Module()
        self.output.dense = _lin(I, D)
        self.output.LayerNorm = nn.LayerNorm(D, eps=eps)


class BlipCaptioner(nn.Module):
    """``BlipForConditionalGeneration`` (vision tower + text decoder + LM head) for greedy, beam-search and sampled captioning on the
    HIP kernels."""

    def __init__(self, text: dict, vision: dict, compute_dtype: str = "fp16"):
        super().__init__()
        if compute_dtype not in ("bf16", "fp16"):
            raise ValueError(f"compute_dtype must be 'bf16' or 'fp16', got {compute_dtype!r}")
        for nm, c in (("text", text), ("vision", vision)):
            if c["hidden_size"] % c["num_attention_heads"] or c["hidden_size"] // c["num_attention_heads"] != 64:
                raise ValueError(f"{nm}: head dim must be 64 (hidden_size / num_attention_heads)")
            if c["hidden_size"] % 128 or c["intermediate_size"] % 128:
                raise ValueError(f"{nm}: hidden_size and intermediate_size must be multiples of 128")
            if c["hidden_act"] != "gelu":
                raise ValueError(f"{nm}: only the erf GELU ('gelu') is implemented, got {c['hidden_act']!r}")
        if text["encoder_hidden_size"] != vision["hidden_size"]:
            raise ValueError("text encoder_hidden_size must equal the vision hidden_size")
        if vision["patch_size"] % 8 or vision["image_size"] % vision["patch_size"] or vision["num_channels"] != 3:
            raise ValueError("vision: 3 channels, patch_size a multiple of 8 dividing image_size")
        self.text_cfg, self.vision_cfg, self.compute_dtype = dict(text), dict(vision), compute_dtype
        Dv, Iv, ps = vision["hidden_size"], vision["intermediate_size"], vision["patch_size"]
        n_pos = (vision["image_size"] // ps) ** 2 + 1
        self.vision_model = nn.Module()
        emb = nn.Module()
        emb.class_embedding = nn.Parameter(torch.randn(1, 1, Dv) * 0.02)
        emb.patch_embedding = nn.Conv2d(3, Dv, kernel_size=ps, stride=ps)
        emb.position_embedding = nn.Parameter(torch.randn(1, n_pos, Dv) * 0.02)
        self.vision_model.embeddings = emb
        self.vision_model.encoder = nn.Module()
        self.vision_model.encoder.layers = nn.ModuleList(
            [_VisionLayer(Dv, Iv, vision["layer_norm_eps"]) for _ in range(vision["num_hidden_layers"])])
        self.vision_model.post_layernorm = nn.LayerNorm(Dv, eps=vision["layer_norm_eps"])
        D, V = text["hidden_size"], text["vocab_size"]
        eps = text["layer_norm_eps"]
        self.text_decoder = nn.Module()
        bert = nn.Module()
        bert.embeddings = nn.Module()
        bert.embeddings.word_embeddings = nn.Embedding(V, D)
        bert.embeddings.position_embeddings = nn.Embedding(text["max_position_embeddings"], D)
        bert.embeddings.LayerNorm = nn.LayerNorm(D, eps=eps)
        bert.encoder = nn.Module()
        bert.encoder.layer = nn.ModuleList([_TextLayer(D, text["encoder_hidden_size"], text["intermediate_size"], eps)
                                            for _ in range(text["num_hidden_layers"])])
        self.text_decoder.bert = bert
        cls = nn.Module()
        cls.predictions = nn.Module()
        cls.predictions.bias = nn.Parameter(torch.zeros(V))
        cls.predictions.transform = nn.Module()
        cls.predictions.transform.dense = _lin(D, D)
        cls.predictions.transform.LayerNorm = nn.LayerNorm(D, eps=eps)
        cls.predictions.decoder = _lin(D, V)
        self.text_decoder.cls = cls
        self._pack = None
        self._pack_key = None
        self._states = {}

    @classmethod
    def from_config(cls, cfg, compute_dtype: str = "fp16", device="cpu") -> "BlipCaptioner":
        """``cfg``: a transformers ``BlipConfig`` or its ``to_dict()``; missing fields take BlipConfig's defaults."""
        text, vision = _section(cfg, "text_config", _TEXT_DEFAULTS), _section(cfg, "vision_config", _VISION_DEFAULTS)
        with torch.device(device):
            return cls(text, vision, compute_dtype)

    # ---- 16-bit GEMM operands (rebuilt when a parameter changed) --------------------------------------------------------------
    def _T16(self):
        return torch.float16 if self.compute_dtype == "fp16" else torch.bfloat16

    def _packed(self):
        params = list(self.parameters())
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self._pack is not None and self._pack_key == key:
            return self._pack
        T16 = self._T16()

        def w16(*ws):
            return torch.cat([w.detach() for w in ws], 0).to(T16).contiguous()

        def f32(*bs):
            return torch.cat([b.detach().reshape(-1) for b in bs], 0).to(F32).contiguous()

        def ln(m):
            return f32(m.weight), f32(m.bias)

        with torch.no_grad():
            vm = self.vision_model
            pe = vm.embeddings.patch_embedding
            pk = {"patch": (w16(pe.weight.reshape(pe.out_channels, -1)), f32(pe.bias)),
                  "cls": f32(vm.embeddings.class_embedding), "pos": f32(vm.embeddings.position_embedding),
                  "post": ln(vm.post_layernorm), "vis": [], "txt": []}
            for L in vm.encoder.layers:
                pk["vis"].append((ln(L.layer_norm1), w16(L.self_attn.qkv.weight), f32(L.self_attn.qkv.bias),
                                  w16(L.self_attn.projection.weight), f32(L.self_attn.projection.bias), ln(L.layer_norm2),
                                  w16(L.mlp.fc1.weight), f32(L.mlp.fc1.bias), w16(L.mlp.fc2.weight), f32(L.mlp.fc2.bias)))
            bert = self.text_decoder.bert
            pk["word"] = f32(bert.embeddings.word_embeddings.weight).view(-1, self.text_cfg["hidden_size"])
            pk["tpos"] = f32(bert.embeddings.position_embeddings.weight).view(-1, self.text_cfg["hidden_size"])
            pk["emb_ln"] = ln(bert.embeddings.LayerNorm)
            for L in bert.encoder.layer:
                sa, ca = L.attention, L.crossattention
                pk["txt"].append(dict(
                    wqkv=w16(sa.self.query.weight, sa.self.key.weight, sa.self.value.weight),
                    bqkv=f32(sa.self.query.bias, sa.self.key.bias, sa.self.value.bias),
                    wo=w16(sa.output.dense.weight), bo=f32(sa.output.dense.bias), ln1=ln(sa.output.LayerNorm),
                    wcq=w16(ca.self.query.weight), bcq=f32(ca.self.query.bias),
                    wckv=w16(ca.self.key.weight, ca.self.value.weight), bckv=f32(ca.self.key.bias, ca.self.value.bias),
                    wco=w16(ca.output.dense.weight), bco=f32(ca.output.dense.bias), ln2=ln(ca.output.LayerNorm),
                    wi=w16(L.intermediate.dense.weight), bi=f32(L.intermediate.dense.bias),
                    wout=w16(L.output.dense.weight), bout=f32(L.output.dense.bias), ln3=ln(L.output.LayerNorm)))
            pr = self.text_decoder.cls.predictions
            V, D = pr.decoder.weight.shape
            Vp = (V + 127) // 128 * 128
            wdec = torch.zeros((Vp, D), dtype=T16, device=pr.decoder.weight.device)
            wdec[:V] = pr.decoder.weight.detach().to(T16)
            bdec = torch.zeros(Vp, dtype=F32, device=wdec.device)
            bdec[:V] = pr.decoder.bias.detach().to(F32)
            pk["head"] = (w16(pr.transform.dense.weight), f32(pr.transform.dense.bias), ln(pr.transform.LayerNorm), wdec, bdec)
        self._pack, self._pack_key = pk, key
        self._states = {}
        return pk

    # ---- vision tower ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def vision_forward(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """``vision_model(pixel_values)[0]`` (after ``post_layernorm``): 16-bit [B * (1 + patches), D]."""
        if not pixel_values.is_cuda:
            raise _lib.MemehipError("BlipCaptioner runs on the HIP device only (no CPU fallback): move the batch with .to(device)")
        vc = self.vision_cfg
        S = vc["image_size"]
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, S, S):
            raise ValueError(f"pixel_values must be [B, 3, {S}, {S}] (the config's image_size; no interpolate_pos_encoding)")
        pk = self._packed()
        B = pixel_values.shape[0]
        D, H, ps, eps = vc["hidden_size"], vc["num_attention_heads"], vc["patch_size"], vc["layer_norm_eps"]
        Np = (S // ps) ** 2
        T16 = self._T16()
        patches = ops.patchify(pixel_values.detach().to(F32).contiguous(), ps, dtype=T16)
        proj = ops.linear_fwd(patches, pk["patch"][0], bias=pk["patch"][1])
        x = torch.empty((B * (Np + 1), D), dtype=T16, device=pixel_values.device)
        ops.vit_assemble_fwd(proj, pk["cls"], pk["pos"], x, B, Np, D)
        for (g1, b1), wqkv, bqkv, wo, bo, (g2, b2), w1, bb1, w2, bb2 in pk["vis"]:
            h, _, _ = ops.layernorm_fwd(x, g1, b1, eps)
            qkv = ops.linear_fwd(h, wqkv, bias=bqkv)
            a, _ = ops.attn_fwd(qkv, None, B, Np + 1, H)
            x = ops.linear_fwd(a, wo, bias=bo, residual=x)
            h, _, _ = ops.layernorm_fwd(x, g2, b2, eps)
            f = ops.linear_fwd(h, w1, bias=bb1, gelu=True)
            x = ops.linear_fwd(f, w2, bias=bb2, residual=x)
        y, _, _ = ops.layernorm_fwd(x, *pk["post"], eps)
        return y

    # ---- decoder state and one step -------------------------------------------------------------------------------------------
    def _state(self, B: int, cap: int, device, K: int = 1, nseq: int = 1):
        """buffers of the decode step for B images of K beams, or of nseq sampled sequences (K = 1): R = B * K * nseq rows, cross
        k / v one copy per image"""
        key = (B, cap, str(device), K, nseq)
        if key in self._states:
            return self._states[key]
        tc, T16 = self.text_cfg, self._T16()
        D, I, H, nl = tc["hidden_size"], tc["intermediate_size"], tc["num_attention_heads"], tc["num_hidden_layers"]
        Ni = (self.vision_cfg["image_size"] // self.vision_cfg["patch_size"]) ** 2 + 1
        Vp = self._pack["head"][3].shape[0]
        e = lambda *s, dt=T16: torch.empty(s, dtype=dt, device=device)
        R = B * K * nseq
        rows = R if K == 1 else B          # rows of the greedy / sampled selection (beam search keeps its own state)
        ns_self, ns_cross = ops.decode_splits(R, H, cap), ops.decode_splits(R, H, Ni)
        st = dict(B=B, K=K, G=K * nseq, R=R, cap=cap, Ni=Ni, ns_self=ns_self, ns_cross=ns_cross,
                  cache=[torch.zeros((R, cap, 2 * D), dtype=T16, device=device) for _ in range(nl)],
                  ckv=[e(B * Ni, 2 * D) for _ in range(nl)],
                  x=e(R, D), x1=e(R, D), s=e(R, D), ctx=e(R, D), q=e(R, D), qkv=e(R, 3 * D), ffn=e(R, I), h=e(R, D),
                  mean=e(R, dt=F32), rstd=e(R, dt=F32), logits=e(R, Vp, dt=F32),
                  ws=e(R * H * max(ns_self, ns_cross, 1) * 66, dt=F32),
                  out_ids=e(rows, cap, dt=I64), next_ids=e(R, dt=I64), finished=e(rows, dt=I32), sv=e(4, dt=I32), graph=None, beam=None,
                  rng=torch.zeros(4, dtype=I32, device=device), u=torch.zeros(R, dtype=F32, device=device))
        self._states = {key: st}          # one live batch shape at a time (the caches are large)
        return st

    def _step(self, st):
        pk, tc = self._pack, self.text_cfg
        B, cap, Ni, G = st["R"], st["cap"], st["Ni"], st["G"]       # B: rows of the step ([image][beam] or [image][sequence]), G per image
        D, H, eps = tc["hidden_size"], tc["num_attention_heads"], tc["layer_norm_eps"]
        beam = st["beam"]
        t = st["sv"][0:1] if beam is None else beam["state"][0:1]
        next_ids = st["next_ids"] if beam is None else beam["next_ids"]
        src = None if beam is None else beam["src"]
        x, x1, s, ctx, q, qkv, ffn, h = (st[k] for k in ("x", "x1", "s", "ctx", "q", "qkv", "ffn", "h"))
        mean, rstd, ws = st["mean"], st["rstd"], st["ws"]
        ops.decode_embed(next_ids, t, pk["word"], pk["tpos"], *pk["emb_ln"], eps, x)
        qkv_flat = qkv.view(-1)
        for lw, cache, ckv in zip(pk["txt"], st["cache"], st["ckv"]):
            cf, kf = cache.view(-1), ckv.view(-1)
            ops.linear_fwd(x, lw["wqkv"], bias=lw["bqkv"], out=qkv)
            ops.attn_decode(qkv, cf, cf[D:], ctx, B, H, cap, 3 * D, cap * 2 * D, 2 * D, D, t_dev=t, kv_new=qkv_flat[D:], ld_new=3 * D,
                            nsplit=st["ns_self"], workspace=ws, src=src)
            ops.linear_fwd(ctx, lw["wo"], bias=lw["bo"], residual=x, out=s)
            ops.layernorm_fwd(s, *lw["ln1"], eps, y=x1, mean=mean, rstd=rstd)
            ops.linear_fwd(x1, lw["wcq"], bias=lw["bcq"], out=q)
            ops.attn_decode(q, kf, kf[D:], ctx, B, H, Ni, D, Ni * 2 * D, 2 * D, D, nsplit=st["ns_cross"], workspace=ws, kv_group=G)
            ops.linear_fwd(ctx, lw["wco"], bias=lw["bco"], residual=x1, out=s)
            ops.layernorm_fwd(s, *lw["ln2"], eps, y=x1, mean=mean, rstd=rstd)
            ops.linear_fwd(x1, lw["wi"], bias=lw["bi"], gelu=True, out=ffn)
            ops.linear_fwd(ffn, lw["wout"], bias=lw["bout"], residual=x1, out=s)
            ops.layernorm_fwd(s, *lw["ln3"], eps, y=x, mean=mean, rstd=rstd)
        wt, bt, lnh, wdec, bdec = pk["head"]
        ops.linear_fwd(x, wt, bias=bt, gelu=True, out=h)
        ops.layernorm_fwd(h, *lnh, eps, y=x1, mean=mean, rstd=rstd)
        Vp = wdec.shape[0]
        ops.gemm_grouped([ops.Gemm(x1, wdec, st["logits"], B, Vp, D, D, D, Vp, bias=bdec)], False, False)
        if beam is None and st["sampling"] is not None:
            ops.sample_step(st["logits"], tc["vocab_size"], st["out_ids"], st["next_ids"], st["finished"], st["sv"], st["P"],
                            tc["sep_token_id"], tc["pad_token_id"], st["sampling"], st["rng"], u_out=st["u"], process=st["process"])
        elif beam is None:
            ops.greedy_step(st["logits"], tc["vocab_size"], st["out_ids"], st["next_ids"], st["finished"], st["sv"], st["P"],
                            tc["sep_token_id"], tc["pad_token_id"], process=st["process"])
        else:
            ops.beam_step(st["logits"], tc["vocab_size"], beam, st["P"], st["length_penalty"], st["early_stopping"], tc["sep_token_id"],
                          process=st["process"])

    def _prepare(self, pixel_values, prompt, cap, num_beams=1, length_penalty=1.0, early_stopping=False, process=None, sampling=None,
                 nseq=1, seed=0):
        """vision tower, cross k / v of every layer, and the step's state for this prompt (int64 [B, P] on the device).
        process: an ``ops.logits_process`` (None: no logits processors, the plain selection kernels).  sampling: an ``ops.sampling``
        (None: greedy decoding or beam search) for nseq sequences per image, rows [image][sequence], drawn under ``seed``."""
        img = self.vision_forward(pixel_values)
        B, P = prompt.shape
        st = self._state(B, cap, pixel_values.device, num_beams, nseq)
        st["sampling"] = sampling
        st["P"], st["length_penalty"], st["early_stopping"] = P, float(length_penalty), early_stopping
        st["process"] = None if ops.process_is_neutral(process) else process
        pkey = None if st["process"] is None else (process.repetition_penalty, process.no_repeat_ngram_size, process.min_length,
                                                   process.min_new_tokens)
        skey = None if sampling is None else (sampling.temperature, sampling.top_k, sampling.top_p)
        # what a captured step has baked in: the decoding mode and its settings, not the seed (the step reads it from st["rng"])
        st["key"] = (P, num_beams, float(length_penalty), early_stopping, pkey, skey)
        D = self.text_cfg["hidden_size"]
        gs = [ops.Gemm(img, lw["wckv"], ckv, img.shape[0], 2 * D, img.shape[1], img.shape[1], img.shape[1], 2 * D, bias=lw["bckv"])
              for lw, ckv in zip(self._pack["txt"], st["ckv"])]
        for i in range(0, len(gs), _lib.MH_GEMM_MAX_GROUP):
            ops.gemm_grouped(gs[i:i + _lib.MH_GEMM_MAX_GROUP], False, False)
        if num_beams > 1:
            # transformers fills beam sequences with `pad_token_id or eos_token_id`: a pad id of 0 (BLIP's) counts as unset there
            fill = self.text_cfg["pad_token_id"] or self.text_cfg["sep_token_id"]
            if st["beam"] is None:
                st["beam"] = ops.beam_state(B, num_beams, cap, prompt, fill, pixel_values.device)
            else:                      # same tensors (a captured step points at them), start values
                fresh = ops.beam_state(B, num_beams, cap, prompt, fill, pixel_values.device)
                for n, v in fresh.items():
                    if isinstance(v, torch.Tensor):
                        st["beam"][n].copy_(v)
            return st
        st["out_ids"].fill_(self.text_cfg["pad_token_id"])
        st["out_ids"][:, :P] = prompt.repeat_interleave(nseq, 0) if nseq > 1 else prompt
        st["next_ids"].copy_(st["out_ids"][:, 0])
        if sampling is not None:
            ops.set_sample_rng(st["rng"], seed)
        st["finished"].zero_()
        st["sv"].zero_()
        return st

    def _run(self, st, steps: int, graph: bool, poll_every: int, record=None, trace=None):
        """``steps`` decode steps (stops early once every row has finished, checked every ``poll_every`` steps).  ``record``: a
        list that receives each step's logits; ``trace``: a list that receives, per step, a dict of copies of the logits the step
        used and of the beam state after it (``ops.beam_state``'s tensors), or for greedy decoding of ``next_ids`` (the chosen
        tokens), ``finished`` and ``state``, and for a sampled run also of ``u``, the uniforms the step drew with."""
        done = st["sv"] if st["beam"] is None else st["beam"]["state"]
        for i in range(steps):
            if i == 0 or not graph:
                self._step(st)
            else:
                if st["graph"] is None or st["graph_key"] != st["key"]:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._step(st)
                    st["graph"], st["graph_key"] = g, st["key"]
                st["graph"].replay()
            if record is not None:
                record.append(st["logits"][:, :self.text_cfg["vocab_size"]].clone())
            if trace is not None:
                if st["beam"] is None:      # greedy / sampled: the tokens the step chose, its finished flags and state words after it
                    snap = dict(next_ids=st["next_ids"].clone(), finished=st["finished"].clone(), state=st["sv"].clone())
                    if st["sampling"] is not None:
                        snap["u"] = st["u"].clone()                # the uniforms the step drew with
                else:
                    snap = {n: v.clone() for n, v in st["beam"].items() if isinstance(v, torch.Tensor) and not n.startswith("cand_")}
                snap["logits"] = st["logits"][:, :self.text_cfg["vocab_size"]].clone()
                trace.append(snap)
            if i + 1 < steps and (i + 1) % poll_every == 0 and int(done[3]) != 0:
                break

    # ---- public surface -------------------------------------------------------------------------------------------------------
    def _prompt(self, pixel_values, input_ids, attention_mask):
        B = pixel_values.shape[0]
        tc = self.text_cfg
        if input_ids is None:
            ids = torch.tensor([[tc["bos_token_id"], tc["sep_token_id"]]], dtype=I64).repeat(B, 1)
        else:
            ids = torch.as_tensor(input_ids).to(I64).clone()
        if ids.dim() != 2 or ids.shape[0] != B or ids.shape[1] < 2:
            raise ValueError("input_ids must be [B, L] with L >= 2 (the processor's prompt ends with [SEP], which generate drops)")
        if attention_mask is not None and bool((torch.as_tensor(attention_mask) == 0).any()):
            raise ValueError("prompt attention masks with zeros are not implemented (every prompt of a batch has the same length)")
        ids[:, 0] = tc["bos_token_id"]
        return ids[:, :-1]

    @torch.no_grad()
    def generate(self, pixel_values: torch.Tensor, input_ids: Optional[torch.Tensor] = None, attention_mask=None,
                 max_new_tokens: int = 20, *, graph: bool = True, poll_every: int = 8, num_beams: int = 1, length_penalty: float = 1.0,
                 early_stopping=False, num_return_sequences: int = 1, do_sample: bool = False, temperature: float = 1.0,
                 top_k: int = 50, top_p: float = 1.0, seed: Optional[int] = None,
                 repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_length: int = 0, min_new_tokens: int = 0,
                 interpolate_pos_encoding: bool = False, _trace=None) -> torch.LongTensor:
        """``BlipForConditionalGeneration.generate(pixel_values, input_ids, attention_mask, max_new_tokens=...)``:
        ``input_ids[:, 0]`` becomes ``bos_token_id``, the last prompt token is dropped, eos is ``sep_token_id``.

        Greedy (``num_beams=1``, the default): rows that emitted eos continue with ``pad_token_id``, and the output ends at the step
        where the last row finished (or after ``max_new_tokens``).

        Beam search (``2 <= num_beams <= 8``, with ``length_penalty`` and ``early_stopping`` False, True or ``"never"``):
        transformers' ``_beam_search`` on the device.  The best finished beam of every image is returned, cut to the prompt plus
        the longest generated length among the returned beams and padded as transformers pads it: with ``pad_token_id or
        eos_token_id``, i.e. with eos where the pad id is 0, as BLIP's is.  Where torch.topk leaves
        a tie open, the lower flat index ``beam * vocab_size + token`` wins (the lower position in the later selections).  The loop
        ends once no image's finished beams can change any more (transformers may run further steps; the result is the same).

        Logits processors, transformers' own in ``_get_logits_processor``'s order, inside the device step (the captured graph
        included): ``repetition_penalty`` (finite, > 0; every distinct token of the row so far, prompt included, is penalised once),
        ``no_repeat_ngram_size``, ``min_length`` (counts the prompt) and ``min_new_tokens`` (integers >= 0).  Greedy decoding
        applies them to the raw f32 logits, beam search to the row's log-softmax before the beam's score is added, as transformers
        does.  With the neutral values (1, 0, 0, 0) the step is exactly the one without them.  Beam search with a processor needs
        ``vocab_size >= 2 * num_beams + prompt + max_new_tokens + 1``, so that the bans leave every beam its candidates.

        ``num_return_sequences = n`` with beam search (``1 <= n <= num_beams``): the n best finished beams of every image, best
        first, as ``[B * n, L]`` rows ordered [image][rank], cut to the prompt plus the longest generated length among the returned
        rows.  A slot that holds no finished beam (the search closed before n beams finished) yields the prompt followed by the
        padding, with length 0.

        Sampling (``do_sample=True``, ``num_beams=1``; defaults ``temperature=1.0``, ``top_k=50`` -- transformers' default generation
        config --, ``top_p=1.0``, ``seed=None``): the greedy loop with ``mh_sample_step`` in place of the argmax, inside the device
        step.  Per row, in transformers' order: the logits processors, ``x / temperature`` (finite, > 0), top-k (an integer >= 0; 0:
        off; ties at the k-th value are all kept), top-p (in (0, 1]; a token is kept iff the mass of the survivors with a strictly
        larger value is below ``top_p`` of the total, so equal values at the boundary are all kept), then one multinomial draw over
        what is kept.  The uniform of a draw is a counter hash of (seed, row, column): the same seed gives the same captions on every
        run, with or without the graph, and a captured step serves every seed (it reads the seed from device memory).  ``seed``: an
        int is used as given (its low 64 bits); ``None`` draws 64 bits from torch's default CPU generator, so ``torch.manual_seed``
        makes a call reproducible.  The stream is not torch.multinomial's: tokens are not those of transformers' sampled ``generate``.
        ``num_return_sequences = n >= 1`` with sampling (``B * n <= 1024``): n captions per image as ``[B * n, L]`` rows ordered
        [image][k]; the vision tower runs once per image, and row ``image * n + k`` is the row of the hash, so the n captions differ
        (and differ from n single calls, whose rows are ``image``).  Without ``do_sample`` the three settings are checked and ignored.

        ``graph=False`` runs the same launches without the hipGraph.  Refused with ``ValueError``: ``num_beams`` outside 1..8,
        ``num_return_sequences`` above num_beams without sampling, ``do_sample=True`` with ``num_beams > 1`` (no beam sampling), values
        of the sampling settings outside their domains, ``interpolate_pos_encoding``, prompt attention masks with zeros, and
        ``num_beams > 1``, sampling or any logits processor for a model or batch that is not on the HIP device (plain greedy calls
        there raise ``MemehipError``: there is no CPU path at all)."""
        if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= 8:
            raise ValueError("num_beams must be an integer from 1 (greedy) to 8")
        nrs = num_return_sequences
        if isinstance(nrs, bool) or not isinstance(nrs, int) or nrs < 1:
            raise ValueError("num_return_sequences must be an integer >= 1")
        if not isinstance(do_sample, bool):
            raise ValueError("do_sample must be True or False")
        if do_sample and num_beams > 1:
            raise ValueError("do_sample=True needs num_beams=1 (beam sampling is not implemented)")
        if nrs > num_beams and not do_sample:
            raise ValueError("num_return_sequences must be <= num_beams (more than one sequence needs beam search or do_sample=True)")
        if not isinstance(early_stopping, bool) and early_stopping != "never":
            raise ValueError("early_stopping must be False, True or 'never'")
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
            raise ValueError("seed must be an integer or None")
        sampling = ops.sampling(temperature, top_k, top_p)                                                      # ValueError if invalid
        sampling = sampling if do_sample else None              # (the three are validated, then ignored, without do_sample)
        process = ops.logits_process(repetition_penalty, no_repeat_ngram_size, min_length, min_new_tokens)      # ValueError if invalid
        on_device = isinstance(pixel_values, torch.Tensor) and pixel_values.is_cuda and next(self.parameters()).is_cuda
        if do_sample and not on_device:
            raise ValueError("sampling (do_sample=True) exists only in the HIP decode step: move the model and batch with .to(device)")
        if num_beams > 1 and not on_device:
            # (the argument is refused, as before beam search existed: the search lives in the device step and nowhere else)
            raise ValueError("beam search (num_beams > 1) exists only in the HIP decode step: move the model and batch with .to(device)")
        if not ops.process_is_neutral(process) and not on_device:
            raise ValueError("repetition_penalty, no_repeat_ngram_size, min_length and min_new_tokens exist only in the HIP decode step: "
                             "move the model and batch with .to(device)")
        if interpolate_pos_encoding:
            raise ValueError("interpolate_pos_encoding is not implemented: pixel_values must have the config's image_size")
        if int(max_new_tokens) < 1 or int(poll_every) < 1:
            raise ValueError("max_new_tokens and poll_every must be >= 1")
        S = self.vision_cfg["image_size"]
        if not isinstance(pixel_values, torch.Tensor) or pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, S, S):
            raise ValueError(f"pixel_values must be [B, 3, {S}, {S}] (the config's image_size; no interpolate_pos_encoding)")
        prompt = self._prompt(pixel_values, input_ids, attention_mask)
        if not pixel_values.is_cuda or not next(self.parameters()).is_cuda:
            raise _lib.MemehipError("BlipCaptioner runs on the HIP device only (no CPU fallback): move the model and batch with .to(device)")
        prompt = prompt.to(pixel_values.device)
        P = prompt.shape[1]
        cap = P + int(max_new_tokens)
        if cap > self.text_cfg["max_position_embeddings"]:
            raise ValueError("prompt + max_new_tokens exceeds max_position_embeddings")
        self._packed()
        if num_beams > 1:
            if self.text_cfg["vocab_size"] < 2 * num_beams:
                raise ValueError("beam search needs vocab_size >= 2 * num_beams")
            if not ops.process_is_neutral(process) and self.text_cfg["vocab_size"] < 2 * num_beams + cap + 1:
                raise ValueError("beam search with logits processors needs vocab_size >= 2 * num_beams + prompt + max_new_tokens + 1")
            st = self._prepare(pixel_values, prompt, cap, num_beams, length_penalty, early_stopping, process)
            self._run(st, P - 1 + int(max_new_tokens), graph, int(poll_every), trace=_trace)
            bs = st["beam"]
            lens = bs["fin_len"].view(-1, num_beams)[:, :nrs]
            return bs["fin_seq"].view(-1, num_beams, cap)[:, :nrs, :P + int(lens.max())].reshape(-1, P + int(lens.max())).to(I64)
        if sampling is None:
            st = self._prepare(pixel_values, prompt, cap, process=process)
        else:
            if prompt.shape[0] * nrs > 1024:
                raise ValueError("sampling: batch * num_return_sequences must be <= 1024")
            if self.text_cfg["vocab_size"] > _lib.MH_PROCESS_MAX_VOCAB:
                raise ValueError(f"sampling needs vocab_size <= {_lib.MH_PROCESS_MAX_VOCAB}")
            if seed is None:
                seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=I64).item())      # torch's default CPU generator
            st = self._prepare(pixel_values, prompt, cap, process=process, sampling=sampling, nseq=nrs, seed=seed)
        self._run(st, P - 1 + int(max_new_tokens), graph, int(poll_every), trace=_trace)
        sv = st["sv"].cpu()
        length = int(sv[3]) if int(sv[3]) else min(cap, int(sv[0]) + 1)
        return st["out_ids"][:, :length].clone()

    @torch.no_grad()
    def teacher_forced_logits(self, pixel_values: torch.Tensor, input_ids: torch.Tensor, graph: bool = False) -> torch.Tensor:
        """f32 [B, L, vocab]: the LM-head logits after each token of ``input_ids`` (used as given, no bos substitution), fed one
        per step through the decode step -- ``text_decoder(input_ids, encoder_hidden_states=vision(pixel_values)[0]).logits``."""
        if not pixel_values.is_cuda:
            raise _lib.MemehipError("BlipCaptioner runs on the HIP device only (no CPU fallback)")
        ids = torch.as_tensor(input_ids).to(I64).to(pixel_values.device)
        B, L = ids.shape
        self._packed()
        st = self._prepare(pixel_values, ids, L + 1)
        rec = []
        self._run(st, L, graph, L + 1, record=rec)
        return torch.stack(rec, 1)
