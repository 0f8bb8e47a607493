"""torchvision ``convnext_tiny`` forward on the HIP kernels: the image features of the SVM baseline.

``baselines/extract_feat.py:52-60,82-85`` builds ``convnext_tiny(weights=ConvNeXt_Tiny_Weights.DEFAULT)``, puts it in eval mode and
takes ``img_model.avgpool(img_model.features(images))`` (768 numbers per image, WITHOUT the classifier's LayerNorm) under
``torch.no_grad()``.  ``ConvNeXtTiny`` holds the same parameters under torchvision's state_dict names
(``features.0.0.weight`` ... ``features.7.2.layer_scale``, ``classifier.0 / .2``) so that checkpoint loads ``strict=True``, and
``pooled_features(image)`` is that expression: forward only, no CPU path.

Launch plan, activations NHWC 16-bit = row matrices ``[B*H*W][C]``:

* stem ``Conv2d(3, 96, 4, stride=4)``: ``mh_patchify_ld`` (4x4 patches, 48 -> 64 columns) + the grouped MFMA GEMM with the bias in
  its epilogue, then ``LayerNorm2d`` = ``mh_layernorm_fwd`` over the channel rows (eps 1e-6);
* CNBlock: ``mh_dwconv_nhwc`` (7x7 depthwise, LDS halo tiles) -> ``mh_layernorm_fwd`` -> GEMM (+bias, erf-GELU in the epilogue) ->
  GEMM (+bias, + the block input as the epilogue's residual operand); ``layer_scale`` is folded into the second Linear's rows
  (``gamma * (W h + b) = (gamma W) h + gamma b``) when the 16-bit weights are packed;
* downsampling ``LayerNorm2d`` + ``Conv2d(C, 2C, 2, stride=2)``: ``mh_layernorm_fwd``, ``mh_im2col_nhwc`` (non-overlapping windows: a
  permutation, 1x the activation bytes) + GEMM (+bias);
* ``AdaptiveAvgPool2d(1)``: ``mh_avgpool_fwd`` (f32).

Training (``ConvNeXtTiny.tower(image) -> f32 [B, dims[-1]]``, the differentiable ``pooled_features``): the same launches leave a typed
tape (``Tape`` / ``StemRec`` / ``BlockRec`` / ``DownRec``) behind, and ONE opaque autograd node walks it backwards, as ``resnet.py`` does.  Per
CNBlock, for ``dout`` at the block output: the weight gradient of the FOLDED second Linear, then ``mh_layer_scale_bwd`` (``dgamma = sum W dW' +
b db'``, ``dW = gamma dW'``: no extra pass over an activation); its dgrad times the GELU derivative the forward epilogue stored
(``MH_GEMM_DERIV_AUX``); weight gradient and dgrad of the first Linear; ``mh_layernorm_bwd``; ``mh_dwconv_nhwc_wgrad``;
``mh_dwconv_nhwc_dgrad`` with ``addend = dout`` (the residual branch joins in its epilogue).  Downsampling layers: wgrad + dgrad GEMM,
``mh_col2im_nhwc``, LayerNorm backward; stem: LayerNorm backward + the wgrad GEMM over the patch matrix (no image gradient); head of the tower:
``mh_avgpool_bwd``.  A weight gradient contracts over up to 10^5 pixel rows into a handful of output tiles, so it goes as up to
``MH_GEMM_MAX_GROUP`` row chunks of one grouped launch, each with its own f32 slab and bias row sum, summed in a fixed order.  The
16-bit gradient stream carries ``grad_stream_scale`` (8192 for fp16), removed where parameter gradients are produced; gradients go
straight into an existing f32 ``.grad`` (``resnet._grad_target``), so ``flatten_parameters`` + the one fused ``memehip.Adam`` take the
tower like the ResNet one.

Limits.  Stochastic depth is not offered: torchvision's train-mode default is 0.1 and timm's is 0; the tower behaves as probability 0.
In fp16 a ``layer_scale`` near torchvision's from-scratch initial value of 1e-6 underflows in the folded 16-bit weight (released
checkpoints have gamma of order 0.1 ... 1): use bf16 to train from scratch.

Stage 1 has 96 channels and the GEMM contracts in tiles of 64: its first Linear runs with K = 128 against a weight whose columns
96..127 are zero, over the LayerNorm output re-pitched to 128 columns whose last 32 are zero (``mh_im2col_nhwc`` with a 1x1
window).  Contracting the pitch-96 rows directly would multiply the next row's first 32 values by those zero columns: a NaN or
Inf in the first pixel of image b+1 then made image b's last pixel, and so its pooled features, NaN (0 x NaN = NaN).  The backward
pads the same way: the second Linear's dgrad contracts over the 96 output channels, so ``dout`` is re-pitched to 128 columns
(``copy2d_words``) against a folded weight with 32 zero rows, and the first Linear's dgrad rows come back from pitch 128 to 96.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import check
from .resnet import _grad_target

F32 = torch.float32
LN_PARTS = 512          # workgroups (= sets of dgamma / dbeta partials) of a LayerNorm backward, at most
WGRAD_CHUNK_ROWS = 256  # a weight gradient's pixel rows go as min(MH_GEMM_MAX_GROUP, rows // this) chunk problems of one grouped launch


def _stream():
    return torch.cuda.current_stream().cuda_stream


class LayerNorm2d(nn.LayerNorm):
    """torchvision.models.convnext.LayerNorm2d: LayerNorm over the channels of an NCHW tensor (parameter holder here)."""


class CNBlock(nn.Module):
    """torchvision.models.convnext.CNBlock: parameter holder with torchvision's names (block.0 dwconv, block.2 LayerNorm,
    block.3 / block.5 Linear, layer_scale [dim,1,1])."""

    def __init__(self, dim: int, layer_scale: float = 1e-6):
        super().__init__()
        self.block = nn.Sequential(
            nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim, bias=True),
            nn.Identity(),                       # Permute([0, 2, 3, 1])
            nn.LayerNorm(dim, eps=1e-6),
            nn.Linear(dim, 4 * dim, bias=True),
            nn.GELU(),
            nn.Linear(4 * dim, dim, bias=True),
            nn.Identity(),                       # Permute([0, 3, 1, 2])
        )
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * layer_scale)


@dataclass
class StemRec:
    """stem: z = patches @ W^T + b, y = LayerNorm2d(z)"""
    patches: torch.Tensor      # [B*h*w, 64] 16-bit, columns (c, i, j) + 16 zero columns
    z: torch.Tensor            # [B*h*w, dims[0]] LayerNorm input
    mean: torch.Tensor
    rstd: torch.Tensor


@dataclass
class BlockRec:
    """one CNBlock: t = dwconv(x), n = LayerNorm(t), hid = GELU(n W1^T + b1), y = x + hid (gamma W2)^T + gamma b2"""
    mod: CNBlock
    x: torch.Tensor            # [M, d] block input
    t: torch.Tensor            # [M, d] dwconv output = LayerNorm input
    mean: torch.Tensor
    rstd: torch.Tensor
    n: torch.Tensor            # [M, d] LayerNorm output (pitch d: the first Linear's weight gradient reads it unpadded)
    dgelu: torch.Tensor        # [M, 4d] GELU'(pre-activation), stored by the forward epilogue
    hid: torch.Tensor          # [M, 4d]
    wt: torch.Tensor           # the packed weights the forward used: tap-major dwconv image, W1 [4d, kp], gamma W2 [kp, 4d] (zero rows past d)
    w1: torch.Tensor
    w2: torch.Tensor


@dataclass
class DownRec:
    """downsampling layer: n = LayerNorm2d(x), y = im2col_2x2(n) @ Wk^T + b"""
    ln: nn.Module
    conv: nn.Module
    x: torch.Tensor            # [M, d]
    mean: torch.Tensor
    rstd: torch.Tensor
    col: torch.Tensor          # [M/4, 4d]
    wk: torch.Tensor           # [2d, 4d] packed weight


@dataclass
class StageRec:
    d: int
    h: int
    w: int
    blocks: List[BlockRec] = field(default_factory=list)
    down: Optional[DownRec] = None


@dataclass
class Tape:
    B: int
    dtype: torch.dtype
    stem: Optional[StemRec] = None
    stages: List[StageRec] = field(default_factory=list)
    pooled: Optional[torch.Tensor] = None
    last_hw: tuple = (0, 0)


class _TowerFn(torch.autograd.Function):
    """Opaque autograd node: the whole ConvNeXt tower forward; backward walks the saved tape."""

    @staticmethod
    def forward(ctx, image, net, *params):
        ctx.net = net
        ctx.tape = net._forward_tape(image)
        return ctx.tape.pooled.clone()

    @staticmethod
    def backward(ctx, d_pooled):
        grads = ctx.net._backward_tape(ctx.tape, d_pooled)
        ctx.tape = None
        return (None, None) + tuple(grads[id(p)] for p in ctx.net._tower_params)


class _GradSink:
    """Where the backward's parameter gradients go, by resnet._grad_target's convention: a kernel that can accumulate writes straight into an
    existing f32 .grad (autograd gets None); the small vectors a kernel can only overwrite (biases, LayerNorm gamma / beta) are produced
    fresh and added to such a .grad in ONE multi-tensor launch at the end (`flush`), or handed to autograd."""

    def __init__(self):
        self.grads = {}
        self._dst, self._src = [], []

    def target(self, *params):
        """-> ([gradient buffer per parameter], accumulate): in place only when EVERY one has a usable .grad (one kernel, one flag)"""
        probe = {}
        got = [_grad_target(p, probe) for p in params]
        acc = all(a for _, a in got)
        bufs = [g if acc else torch.empty_like(p) for p, (g, _) in zip(params, got)]
        for p, b in zip(params, bufs):
            self.grads[id(p)] = None if acc else b
        return bufs, acc

    def fresh(self, p, g):
        """`g`: this step's whole gradient of `p` in a buffer of its own"""
        dst, acc = _grad_target(p, {})
        if acc:
            self._dst.append(dst)
            self._src.append(g.reshape(dst.shape))
            self.grads[id(p)] = None
        else:
            self.grads[id(p)] = g.reshape(p.shape)

    def flush(self):
        if self._dst:
            torch._foreach_add_(self._dst, self._src)
        self._dst, self._src = [], []


class ConvNeXtTiny(nn.Module):
    """``convnext_tiny`` (depths 3-3-9-3, widths 96-192-384-768).  ``pooled_features(image f32 [B,3,H,W]) -> f32 [B, 768]`` is the
    reference's ``avgpool(features(image))``; ``forward`` adds the classifier (LayerNorm2d + Linear) for completeness; ``tower(image)`` is
    ``pooled_features`` with a backward (module docstring: no stochastic depth; fp16 needs a layer_scale the 16-bit weight can hold).
    ``grad_stream_scale``: the factor on the 16-bit gradient stream (0: 8192 for fp16, 1 for bf16)."""

    def __init__(self, num_classes: int = 1000, compute_dtype: str = "fp16", depths=(3, 3, 9, 3), dims=(96, 192, 384, 768),
                 layer_scale: float = 1e-6, seed: int = 0, grad_stream_scale: float = 0.0):
        super().__init__()
        if compute_dtype not in ("bf16", "fp16"):
            raise ValueError(f"compute_dtype must be 'bf16' or 'fp16', got {compute_dtype!r}")
        torch.manual_seed(seed)
        self.compute_dtype = compute_dtype
        self.gscale = float(grad_stream_scale) if grad_stream_scale else (8192.0 if compute_dtype == "fp16" else 1.0)
        self.depths, self.dims = tuple(depths), tuple(dims)
        layers: List[nn.Module] = [nn.Sequential(nn.Conv2d(3, dims[0], kernel_size=4, stride=4, bias=True), LayerNorm2d(dims[0], eps=1e-6))]
        for si, (n, d) in enumerate(zip(depths, dims)):
            layers.append(nn.Sequential(*[CNBlock(d, layer_scale) for _ in range(n)]))
            if si + 1 < len(dims):
                layers.append(nn.Sequential(LayerNorm2d(d, eps=1e-6), nn.Conv2d(d, dims[si + 1], kernel_size=2, stride=2)))
        self.features = nn.Sequential(*layers)
        # (num_classes=0: no classifier, forward = the pooled features -- what timm's reset_classifier(0) leaves of a backbone)
        self.classifier = nn.Sequential(LayerNorm2d(dims[-1], eps=1e-6), nn.Flatten(1), nn.Linear(dims[-1], num_classes)) if num_classes > 0 else nn.Identity()
        for m in self.modules():          # torchvision's initialisation
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        self._pack = None
        self._pack_key = None
        self.feature_dim = self.dims[-1]
        self._tower_params: List[nn.Parameter] = list(self.features.parameters())

    # ---- 16-bit / tap-major weight images (rebuilt when a parameter changed) ------------------------------------------------
    def _lib(self):
        return _lib.load(self.compute_dtype)

    def _packed(self, T16):
        params = list(self.parameters())
        key = tuple((p.data_ptr(), p._version) for p in params) + (T16,)
        if self._pack is not None and self._pack_key == key:
            return self._pack
        lib = self._lib()
        dev = params[0].device
        pk = {}
        with torch.no_grad():
            conv, ln = self.features[0][0], self.features[0][1]
            c0 = conv.out_channels
            w = torch.zeros((c0, 64), dtype=T16, device=dev)          # (c, i, j) feature order of mh_patchify_ld, 48 -> 64 columns
            w[:, :48] = conv.weight.detach().reshape(c0, 48).to(T16)
            pk["stem"] = (w, conv.bias.detach().to(F32).contiguous(), ln.weight.detach().to(F32).contiguous(), ln.bias.detach().to(F32).contiguous())
            li = 1
            for si, (n, d) in enumerate(zip(self.depths, self.dims)):
                blocks = []
                kp = (d + 63) // 64 * 64
                for blk in self.features[li]:
                    dw, lnb, fc1, fc2 = blk.block[0], blk.block[2], blk.block[3], blk.block[5]
                    wt = torch.empty((49, d), dtype=F32, device=dev)
                    wsrc = dw.weight.detach().to(F32).contiguous()
                    check(lib.mh_dwconv_weight_pack(wsrc.data_ptr(), wt.data_ptr(), d, 7, _stream()), "mh_dwconv_weight_pack")
                    w1 = torch.zeros((4 * d, kp), dtype=T16, device=dev)
                    w1[:, :d] = fc1.weight.detach().to(T16)
                    gamma = blk.layer_scale.detach().to(F32).reshape(d)
                    w2 = torch.zeros((kp, 4 * d), dtype=T16, device=dev)      # rows d..kp-1 zero: the dgrad contracts over kp output channels
                    w2[:d] = (gamma[:, None] * fc2.weight.detach().to(F32)).to(T16)
                    b2 = (gamma * fc2.bias.detach().to(F32)).contiguous()
                    blocks.append((wt, dw.bias.detach().to(F32).contiguous(), lnb.weight.detach().to(F32).contiguous(),
                                   lnb.bias.detach().to(F32).contiguous(), w1, fc1.bias.detach().to(F32).contiguous(), w2, b2))
                pk[("blocks", si)] = blocks
                li += 1
                if si + 1 < len(self.dims):
                    lnd, cv = self.features[li][0], self.features[li][1]
                    d2 = cv.out_channels
                    wk = torch.empty((d2, 4 * d), dtype=T16, device=dev)          # [Cout][(kh, kw, c)]: mh_im2col_nhwc's column order
                    wsrc = cv.weight.detach().to(F32).contiguous()
                    check(lib.mh_conv_weight_pack(wsrc.data_ptr(), wk.data_ptr(), d2, d, 2, 2, d, 4 * d, _stream()), "mh_conv_weight_pack")
                    pk[("down", si)] = (lnd.weight.detach().to(F32).contiguous(), lnd.bias.detach().to(F32).contiguous(), wk,
                                        cv.bias.detach().to(F32).contiguous())
                    li += 1
        self._pack, self._pack_key = pk, key
        return pk

    # ---- launches -------------------------------------------------------------------------------------------------------------
    def _feature_map(self, image: torch.Tensor, tape: Optional[Tape] = None):
        """-> (x 16-bit [B*h*w][768], B, h, w): ``features(image)`` in NHWC rows.  With a `tape` (a Tape's B / dtype are filled in here) the
        SAME launches additionally leave what the backward reads: statistics, the GELU derivative, every layer's input."""
        if not image.is_cuda:
            raise _lib.MemehipError("ConvNeXtTiny runs on the HIP device only (no CPU fallback): move the batch with .to(device)")
        B, Cc, H, W = image.shape
        step = 4 << (len(self.dims) - 1)          # the stem's 4 and a factor 2 per downsampling layer: 32 for convnext_tiny
        if Cc != 3 or H % step or W % step:
            raise ValueError(f"ConvNeXtTiny expects [B, 3, H, W] images with H and W multiples of {step}")
        lib = self._lib()
        T16 = torch.float16 if self.compute_dtype == "fp16" else torch.bfloat16
        pk = self._packed(T16)
        dev = image.device
        img = image.detach().to(F32).contiguous()
        w0, b0, g0, be0 = pk["stem"]
        patches = ops.patchify(img, 4, dtype=T16, ld=64)
        h, w = H // 4, W // 4
        z = ops.linear_fwd(patches, w0, bias=b0)
        x, mean, rstd = ops.layernorm_fwd(z, g0, be0, 1e-6)
        if tape is not None:
            tape.B, tape.dtype, tape.stem = B, T16, StemRec(patches, z, mean, rstd)
        li = 1
        for si, d in enumerate(self.dims):
            M = B * h * w
            kp = (d + 63) // 64 * 64
            stage = StageRec(d, h, w)
            for blk, (wt, bdw, g, be, w1, b1, w2, b2) in zip(self.features[li], pk[("blocks", si)]):
                t = torch.empty((M, d), dtype=T16, device=dev)
                check(lib.mh_dwconv_nhwc(x.data_ptr(), wt.data_ptr(), bdw.data_ptr(), t.data_ptr(), B, h, w, d, 7, _stream()), "mh_dwconv_nhwc")
                n, mean, rstd = ops.layernorm_fwd(t, g, be, 1e-6)
                n_in = n
                if kp != d:      # 96 channels: LayerNorm rows re-pitched to 128 with zero columns (1x1 im2col), contracted over K = 128
                    n_in = torch.empty((M, kp), dtype=T16, device=dev)
                    check(lib.mh_im2col_nhwc(n.data_ptr(), n_in.data_ptr(), B, h, w, d, 1, 1, 1, 0, kp, _stream()), "mh_im2col_nhwc")
                # (the tape asks the epilogue for GELU'(pre-activation) beside the activation: the same exponential, the same hid)
                dgelu = None if tape is None else torch.empty((M, 4 * d), dtype=T16, device=dev)
                hid = ops.linear_fwd(n_in, w1, bias=b1, gelu=True, aux=dgelu, deriv_aux=tape is not None)
                y = ops.linear_fwd(hid, w2[:d], bias=b2, residual=x)
                if tape is not None:
                    stage.blocks.append(BlockRec(blk, x, t, mean, rstd, n, dgelu, hid, wt, w1, w2))
                x = y
            li += 1
            if si + 1 < len(self.dims):
                g, be, wk, bk = pk[("down", si)]
                n, mean, rstd = ops.layernorm_fwd(x, g, be, 1e-6)
                col = torch.empty((M // 4, 4 * d), dtype=T16, device=dev)
                check(lib.mh_im2col_nhwc(n.data_ptr(), col.data_ptr(), B, h, w, d, 2, 2, 2, 0, 4 * d, _stream()), "mh_im2col_nhwc")
                if tape is not None:
                    stage.down = DownRec(self.features[li][0], self.features[li][1], x, mean, rstd, col, wk)
                x = ops.linear_fwd(col, wk, bias=bk)
                h, w = h // 2, w // 2
                li += 1
            if tape is not None:
                tape.stages.append(stage)
        return x, B, h, w

    def _pool(self, x, B, h, w):
        C = self.dims[-1]
        pooled = torch.empty((B, C), dtype=F32, device=x.device)
        check(self._lib().mh_avgpool_fwd(x.data_ptr(), pooled.data_ptr(), B, h * w, C, _stream()), "mh_avgpool_fwd")
        return pooled

    # ---- training: tape forward + backward --------------------------------------------------------------------------------------
    def _forward_tape(self, image: torch.Tensor) -> Tape:
        tape = Tape(0, F32)
        # the weight images are packed anew: a fused optimizer step writes the parameters without touching their version counters, which is
        # all the cache of _packed can see -- and the images of a training forward are not left behind for a later cached one
        self._pack_key = None
        x, B, h, w = self._feature_map(image, tape)
        self._pack_key = None
        tape.pooled, tape.last_hw = self._pool(x, B, h, w), (h, w)
        return tape

    def _wgrad(self, lib, dy, x, K):
        """The weight-gradient GEMM dy^T x[:, :K] over the pixel rows, cut into up to MH_GEMM_MAX_GROUP row chunks of ONE grouped launch (few
        output tiles, a contraction of up to 10^5 rows) -> (slabs f32 [n][N][K], bias gradient f32 [N], n); both carry 1 / gscale."""
        T, N = dy.shape
        n = max(1, min(_lib.MH_GEMM_MAX_GROUP, T // WGRAD_CHUNK_ROWS))
        rows = -(-T // n)
        slabs = torch.empty((n, N, K), dtype=F32, device=dy.device)
        rs = torch.empty((2, n, N), dtype=F32, device=dy.device)          # ([1]: unused half of the colsum_partials layout)
        probs = []
        for s in range(n):
            r0, r1 = s * rows, min(T, (s + 1) * rows)
            probs.append(ops.Gemm(dy[r0:r1], x[r0:r1], slabs[s], N, K, r1 - r0, dy.stride(0), x.stride(0), K, rowsum=rs[0, s], alpha=1.0 / self.gscale))
        ops.gemm_grouped(probs, True, True)
        if n == 1:
            return slabs, rs[0, 0], 1
        db = torch.empty(N, dtype=F32, device=dy.device)
        ops.colsum_partials([(rs, db, None)], n, N)
        return slabs, db, n

    @staticmethod
    def _finish_job(job, slabs, n, g, cout, cin, k, cp, ldk, acc):
        job.slabs, job.g = slabs.data_ptr(), g.data_ptr()
        job.Cout, job.Cin, job.KH, job.KW, job.Cp, job.ldk = cout, cin, k, k, cp, ldk
        job.nsplit, job.accumulate, job.scale = n, int(acc), 1.0

    def _ln_bwd(self, dy, x, ln, mean, rstd, sink):
        """LayerNorm backward over channel rows -> dx; gamma / beta gradients through colsum_partials (minus the stream scale)"""
        rows, D = x.shape
        n_part = max(1, min(LN_PARTS, (rows + 3) // 4))
        part = torch.empty((2, n_part, D), dtype=F32, device=x.device)
        dx = ops.layernorm_bwd(dy, x, ln.weight, mean, rstd, part)
        dg, db = torch.empty(D, dtype=F32, device=x.device), torch.empty(D, dtype=F32, device=x.device)
        ops.colsum_partials([(part, dg, db)], n_part, D, scale=1.0 / self.gscale)
        sink.fresh(ln.weight, dg)
        sink.fresh(ln.bias, db)
        return dx

    def _block_bwd(self, lib, rec: BlockRec, dout, B, h, w, d, sink):
        """dout [M, d] at the block output -> the gradient at the block input (the residual branch included)"""
        M, kp, dev, T16 = B * h * w, rec.w1.shape[1], dout.device, dout.dtype
        dw, ln, fc1, fc2 = rec.mod.block[0], rec.mod.block[2], rec.mod.block[3], rec.mod.block[5]
        # 1. the folded second Linear's weight gradient dW' = dout^T hid, db' = colsum(dout), then layer_scale / W2 / b2 from them
        s2, dbp, n2 = self._wgrad(lib, dout, rec.hid, 4 * d)
        # 2. its dgrad times GELU' (the contraction runs over kp >= d output channels: dout re-pitched, the weight's extra rows are zero)
        dout_p = dout
        if kp != d:
            dout_p = torch.empty((M, kp), dtype=T16, device=dev)
            ops.copy2d_words(dout, d // 2, dout_p, kp // 2, M, d // 2, kp // 2)
        dh = ops.linear_dgrad(dout_p, rec.w2, mul=rec.dgelu, deriv_aux=True)
        # 3. the first Linear: weight gradient over the unpadded LayerNorm output, dgrad back to pitch d
        s1, db1, n1 = self._wgrad(lib, dh, rec.n, d)
        sink.fresh(fc1.bias, db1)
        (g1,), acc1 = sink.target(fc1.weight)
        dWp = torch.empty((d, 4 * d), dtype=F32, device=dev)
        jobs = (_lib.MhConvWgradJob * 2)()
        self._finish_job(jobs[0], s2, n2, dWp, d, 4 * d, 1, 4 * d, 4 * d, False)
        self._finish_job(jobs[1], s1, n1, g1, 4 * d, d, 1, d, d, acc1)
        check(lib.mh_conv_wgrad_finish_batched(jobs, 2, _stream()), "mh_conv_wgrad_finish_batched")
        (g2, gb2, gls), acc2 = sink.target(fc2.weight, fc2.bias, rec.mod.layer_scale)
        ops.layer_scale_bwd(fc2.weight, fc2.bias, rec.mod.layer_scale.view(d), dWp, dbp, gls.view(d), dW=g2, db=gb2, accum=acc2)
        dn = ops.linear_dgrad(dh, rec.w1)
        if kp != d:
            dn_p, dn = dn, torch.empty((M, d), dtype=T16, device=dev)
            ops.copy2d_words(dn_p, kp // 2, dn, d // 2, M, d // 2, d // 2)
        # 4. LayerNorm, 5. + 6. the depthwise convolution; the residual branch's dout joins in the dgrad epilogue
        dt = self._ln_bwd(dn, rec.t, ln, rec.mean, rec.rstd, sink)
        (gdw, gdb), accd = sink.target(dw.weight, dw.bias)
        ops.dwconv_wgrad(rec.x, dt, gdw, gdb, B, h, w, scale=1.0 / self.gscale, accum=accd)
        return ops.dwconv_dgrad(dt, rec.wt, B, h, w, addend=dout)

    def _backward_tape(self, tape: Tape, d_pooled: torch.Tensor):
        lib, B, T16, dev = self._lib(), tape.B, tape.dtype, d_pooled.device
        sink = _GradSink()
        h, w = tape.last_hw
        dx = torch.empty((B * h * w, self.dims[-1]), dtype=T16, device=dev)
        dp32 = d_pooled.to(F32).contiguous()
        check(lib.mh_avgpool_bwd(dp32.data_ptr(), dx.data_ptr(), B, h * w, self.dims[-1], self.gscale, _stream()), "mh_avgpool_bwd")
        for stage in reversed(tape.stages):
            d, h, w = stage.d, stage.h, stage.w
            M = B * h * w
            if stage.down is not None:      # dx: [M/4, 2d] at the downsampling convolution's output
                dn = stage.down
                slabs, dbias, n = self._wgrad(lib, dx, dn.col, 4 * d)
                sink.fresh(dn.conv.bias, dbias)
                (gk,), acc = sink.target(dn.conv.weight)
                jobs = (_lib.MhConvWgradJob * 1)()
                self._finish_job(jobs[0], slabs, n, gk, 2 * d, d, 2, d, 4 * d, acc)      # [(kh, kw, c)] columns -> [Cout][Cin][2][2]
                check(lib.mh_conv_wgrad_finish_batched(jobs, 1, _stream()), "mh_conv_wgrad_finish_batched")
                dcol = ops.linear_dgrad(dx, dn.wk)
                dnorm = torch.empty((M, d), dtype=T16, device=dev)
                check(lib.mh_col2im_nhwc(dcol.data_ptr(), dnorm.data_ptr(), B, h, w, d, 2, 2, 2, 0, 4 * d, _stream()), "mh_col2im_nhwc")
                dx = self._ln_bwd(dnorm, dn.x, dn.ln, dn.mean, dn.rstd, sink)
            for rec in reversed(stage.blocks):
                dx = self._block_bwd(lib, rec, dx, B, h, w, d, sink)
        conv, ln = self.features[0][0], self.features[0][1]
        dz = self._ln_bwd(dx, tape.stem.z, ln, tape.stem.mean, tape.stem.rstd, sink)
        slabs, dbias, n = self._wgrad(lib, dz, tape.stem.patches, 64)
        sink.fresh(conv.bias, dbias)
        (g0,), acc = sink.target(conv.weight)
        jobs = (_lib.MhConvWgradJob * 1)()
        self._finish_job(jobs[0], slabs, n, g0, self.dims[0], 48, 1, 64, 64, acc)          # the first 48 of 64 columns, already (c, i, j)
        check(lib.mh_conv_wgrad_finish_batched(jobs, 1, _stream()), "mh_conv_wgrad_finish_batched")
        sink.flush()
        return sink.grads

    def tower(self, image: torch.Tensor) -> torch.Tensor:
        """``pooled_features(image)`` with a backward: f32 [B, dims[-1]] (= ``feature_dim``).  Under ``torch.no_grad()`` it is the plain
        forward.  Stochastic depth is not offered (probability 0: timm's default; torchvision's train-mode default is 0.1)."""
        if torch.is_grad_enabled():
            return _TowerFn.apply(image, self, *self._tower_params)
        self._pack_key = None
        x, B, h, w = self._feature_map(image)
        self._pack_key = None
        return self._pool(x, B, h, w)

    @torch.no_grad()
    def pooled_features(self, image: torch.Tensor) -> torch.Tensor:
        """``img_model.avgpool(img_model.features(image)).flatten(1)`` (baselines/extract_feat.py:58): f32 [B, 768]."""
        x, B, h, w = self._feature_map(image)
        return self._pool(x, B, h, w)

    @torch.no_grad()
    def forward(self, image: torch.Tensor) -> torch.Tensor:
        """logits [B, num_classes]: classifier = LayerNorm2d -> Flatten -> Linear on the pooled features (eval only)."""
        from . import fused
        pooled = self.pooled_features(image)
        if isinstance(self.classifier, nn.Identity):
            return pooled
        ln, fc = self.classifier[0], self.classifier[2]
        T16 = torch.float16 if self.compute_dtype == "fp16" else torch.bfloat16
        y, _, _ = ops.layernorm_fwd(pooled.to(T16), ln.weight.detach().to(F32).contiguous(), ln.bias.detach().to(F32).contiguous(), 1e-6)
        return fused.linear(y.to(F32), fc.weight, fc.bias)
