"""ResNet image towers on the HIP path: ResNet-50 (BASELINE config 2; the organizers' image encoder:
``models.resnet50(pretrained=True)`` -> 1000 logits -> ``Linear(1000, 512)``, Multimodal_example_task2C.txt:164-165,183-184) and the
basic-block ResNet-18 / 34 (the image tower of the submitted Subtask-2C model: ``timm.create_model("resnet18")`` +
``reset_classifier(0)`` -> 512 features, example_scripts/Multimodal_example_task2C.py:569-574).

``ResNet50`` has torchvision's module tree and state_dict keys (``conv1.weight``, ``bn1.running_mean``,
``layer3.4.conv2.weight``, ``layer2.0.downsample.0.weight``, ``fc.bias`` ...): the ``nn.Conv2d / nn.BatchNorm2d / nn.Linear``
submodules only HOLD the parameters and running statistics; the arithmetic runs in libmemehip:

* activations NHWC 16-bit (a [B*H*W][C] matrix); every convolution is an IMPLICIT GEMM on the MFMA tile (``mh_conv_fwd``:
  the im2col matrix exists only as LDS-DMA source addresses, nothing is materialised); weights are re-packed to
  ``[Cout][(kh,kw,c)]`` 16-bit every forward (150 MB of traffic);
* train-mode BatchNorm2d with per-replica batch statistics (the reference uses plain BN): the statistics come from
  the convolution epilogue's per-tile column sums (``mh_bn2d_fwd_parts``: no pass over the activation), the normalisation is
  fused with the residual add and the ReLU; max pool, global average pool, the 2048 -> 1000 classifier in exact f32;
* the backward is one opaque autograd node over a typed tape (``Tape``): ``mh_conv_wgrad``, the input gradient by the route
  ``dgrad_route`` names (``mh_conv_dgrad``; the strided 1x1 downsamples keep the dgrad GEMM + ``mh_col2im_nhwc`` -- except next to a
  basic block's 3x3 / 2 conv1, where ``pairs_with`` sends both gradients through one ``mh_conv_dgrad_pair`` launch), BatchNorm
  backward; ``ResNet50.options`` (``TowerOptions``) holds its A/B switches;
* ``ResNeXt50_32x4d`` (torchvision ``resnext50_32x4d``, Kevin's Subtask-2B zoo: example_scripts/Untitled-2.py:210-237) is the same walk: a
  bottleneck's grouped 3x3 (``_Conv.grouped``) packs with ``mh_gconv_weight_pack`` and runs ``mh_gconv_fwd`` (BatchNorm partials in its
  epilogue too) / ``mh_gconv_dgrad`` / ``mh_gconv_wgrad`` (straight into the f32 ``.grad``); ``dgrad_route`` names that route ``GROUPED``, so
  it takes no BatchNorm epilogue and no pairing by the existing rules;
* ``SEResNeXt50_32x4d`` (timm ``seresnext50_32x4d``, the zoo's first entry: example_scripts/Untitled-2.py:182-207) adds a squeeze-and-excitation
  gate (``SEModule``) between every bottleneck's bn3 and the residual add.  An SE block takes the plain routes around five small kernels
  (csrc/se.hip): bn3 stores ``u`` with no residual and no ReLU, then ``mh_avgpool_fwd`` / ``mh_se_gate_fwd`` / ``mh_se_apply_fwd``; backward
  ``mh_se_apply_bwd_reduce`` / ``mh_se_gate_bwd`` / ``mh_se_apply_bwd`` and the ordinary unmasked ``mh_bn2d_bwd``.  The conv1 ABOVE an SE
  block never takes the block-out epilogue (``epilogue_takes_bn(..., below_se=True)``): no BatchNorm sits directly under that ReLU;
* the 16-bit gradient stream carries ``grad_stream_scale`` (8192 for fp16), removed where parameter gradients are produced.

``_ConvTower`` holds that machinery -- ONE forward and ONE backward walk over (conv, BatchNorm) units; a family (``_ResNet``: torchvision's
names; ``HFResNetModel``: transformers') only builds its parameter holders from a stage list (``stage_blocks``) and hands them to ``_wire``.

``ResNetClassifier`` is the ResNet-50 (/ 18 / 34) surface of BASELINE config 2 under the Subtask-2B Trainer protocol
(ResNet_example_task2B.py:206-221): ``model(pixel_values=..., labels=...)`` returns ``(loss, logits)``.  The model that example itself
trains -- ``ResNetForImageClassification(ResNetConfig(num_channels=1, layer_type="basic", depths=[2, 2], hidden_sizes=[32, 64]))``,
:146-154 -- is ``HFResNetForImageClassification``: transformers' module tree and state_dict on the same walk.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib, fused, ops
from ._lib import check
from .model import CrossEntropyLoss

F32 = torch.float32
WGRAD_TILES = 256      # split-K tile target of an ungrouped weight gradient (512 / 384 / 256 / 192: 7.78 / 7.74 / 7.74 / 7.72 ms per step; 256 halves the slabs)
GEMM, IMPLICIT, COL2IM, GROUPED = "gemm", "implicit", "gemm + col2im", "grouped"      # the input-gradient routes


@dataclass(frozen=True)
class TowerOptions:
    """A/B switches of the tower's backward (``ResNet50.options``); every default is the measured winner."""
    bn_bwd_fuse: bool = True         # a BatchNorm backward's ReLU mask + statistics in the epilogue of the dgrad that produces its dy
    block_out_fuse: bool = True      # ... and, for a block's bn3, the residual merge too, in the conv1 epilogue of the block above (needs bn_bwd_fuse)
    strided_dgrad: bool = True       # 3x3 / 2 input gradient as four parity classes of mh_conv_dgrad (off: GEMM + col2im)
    # weight gradients launched together (1: one launch each), clamped to MH_CONV_MAX_GROUP.  6 since the conv kernels deal every problem's
    wgrad_group: int = 6             # tiles to all eight XCDs (round 4, second session: 6.29 -> 6.24 ms; with one run over the concatenated tile list 4 was the best)
    # a stage's first BasicBlock: the 1x1 / 2 downsample's input gradient as a second K segment of the 3x3 / 2 conv1's centre-tap parity class
    pair_dgrad: bool = True          # (mh_conv_dgrad_pair; off: GEMM + col2im, then added).  ResNet-50 has no such pair.


def dgrad_route(cv, H, W, opts: TowerOptions) -> str:
    """The input-gradient route of `cv` (a _Conv: geometry only) on an H x W input.  GEMM: a 1x1 / stride 1 is the plain GEMM.
    IMPLICIT: mh_conv_dgrad -- stride 1, or k x k (k > 1) / stride 2 on an even image as four parity-class problems in one launch
    (3 layers of ResNet-50; round 4).  COL2IM: dgrad GEMM into a per-tap panel + mh_col2im_nhwc (the 3 strided 1x1 downsamples).
    GROUPED: mh_gconv_dgrad, a grouped 3x3 (ResNeXt's conv2) -- a gather per input pixel with no BatchNorm epilogue and no pairing."""
    if cv.grouped:
        return GROUPED
    if cv.direct and cv.cout % 64:
        return GEMM
    parity = cv.stride == 2 and cv.kh > 1 and H % 2 == 0 and W % 2 == 0 and opts.strided_dgrad
    if (cv.stride == 1 or parity) and cv.kh == cv.kw and cv.cout % 64 == 0:
        return IMPLICIT
    return COL2IM


def pairs_with(cv, ds, H, W, opts: TowerOptions) -> bool:
    """Whether the input gradients of `cv` (k x k / 2) and `ds` (1x1 / 2 / pad 0), two _Conv that read the same H x W tensor, go as ONE
    mh_conv_dgrad_pair launch: cv by parity classes (so an even image), both on the (H/2) x (W/2) output grid, ds.cout % 64 == 0."""
    return (opts.pair_dgrad and ds.kh == 1 and ds.kw == 1 and ds.stride == 2 and ds.pad == 0 and ds.cout % 64 == 0 and ds.cp == cv.cp
            and cv.stride == 2 and cv.kh > 1 and dgrad_route(cv, H, W, opts) == IMPLICIT and cv.out_hw(H, W) == (H // 2, W // 2))


def epilogue_takes_bn(cv, H, W, opts: TowerOptions, block_out: bool = False, below_se: bool = False) -> bool:
    """Whether cv's dgrad epilogue does the backward masking + statistics of the BatchNorm (+ReLU) that produced cv's input (only
    the implicit route has that epilogue); `block_out`: cv is a block's conv1, the BatchNorm the bn3 + residual of the block below.
    `below_se`: that block is a squeeze-and-excitation block -- its output is relu(u * s + shortcut), so the ReLU's mask and the statistics
    do not belong to a BatchNorm directly under it and the gate needs the FULL gradient of the output: never the block_out form."""
    return (opts.bn_bwd_fuse and (opts.block_out_fuse or not block_out) and not (block_out and below_se)
            and dgrad_route(cv, H, W, opts) == IMPLICIT)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _grad_target(p: nn.Parameter, grads: dict):
    """Where a parameter's gradient is written: straight into an existing f32 .grad (accumulated by the kernel; autograd gets
    None for it -- no add launch per parameter), or a fresh tensor handed to autograd."""
    g = p.grad
    acc = g is not None and g.dtype == F32 and g.is_contiguous() and g.device == p.device
    g = g if acc else torch.empty_like(p)
    grads[id(p)] = None if acc else g
    return g, acc


def _grad_targets(params, grads: dict):
    """_grad_target for parameters that ONE launch writes with one accumulate flag: (targets, accumulate) -- in place only when every one of
    them has a usable .grad, else fresh tensors for all."""
    out = [_grad_target(p, grads) for p in params]
    if len({acc for _, acc in out}) == 1:
        return [g for g, _ in out], out[0][1]
    fresh = [torch.empty_like(p) for p in params]
    for p, g in zip(params, fresh):
        grads[id(p)] = g
    return fresh, False


def _bn_epilogue(below, part, addend=None, y_mask=None):
    """The MhConvBnBwd of a dgrad whose dx is the dy of the BatchNorm (+ReLU) of tape record `below`: mask it, leave its two backward sums per tile
    in `part`.  `addend`: a gradient added before the mask; `y_mask`: the stored output whose sign is the mask (else recomputed from z)."""
    f, m = _lib.MhConvBnBwd(), below.bn.mod
    f.z, f.mean, f.rstd = below.z.data_ptr(), below.mean.data_ptr(), below.rstd.data_ptr()
    f.gamma, f.beta, f.part, f.relu = m.weight.data_ptr(), m.bias.data_ptr(), part.data_ptr(), int(below.relu)
    f.addend = None if addend is None else addend.data_ptr()
    f.y_mask = None if y_mask is None else y_mask.data_ptr()
    return f


class _Conv:
    """One convolution's geometry + launches."""

    def __init__(self, mod: nn.Conv2d, cin_pad: Optional[int] = None):
        self.mod = mod
        self.cout, self.cin = mod.out_channels, mod.in_channels
        self.kh, self.kw = mod.kernel_size
        self.stride, self.pad = mod.stride[0], mod.padding[0]
        self.groups = mod.groups
        self.cp = cin_pad or self.cin                      # channels of the NHWC input (3 -> 8 for the stem)
        k = self.kh * self.kw * self.cp
        self.ldk = (k + 63) // 64 * 64                     # GEMM contraction (multiple of 64)
        self.direct = self.kh == 1 and self.kw == 1 and self.stride == 1 and self.ldk == self.cp

    @property
    def grouped(self) -> bool:
        """THE route property: a grouped convolution (ResNeXt's 3x3 conv2) packs with mh_gconv_weight_pack and runs mh_gconv_fwd / dgrad /
        wgrad; it never enters the dense pack jobs, the deferred weight-gradient queue or dgrad_route's three dense routes."""
        return self.groups > 1

    def out_hw(self, H, W):
        return (H + 2 * self.pad - self.kh) // self.stride + 1, (W + 2 * self.pad - self.kw) // self.stride + 1

    def geom(self, B, H, W):
        g = _lib.MhConvGeom()
        g.B, g.H, g.W, g.C, g.KH, g.KW, g.stride, g.pad, g.Cout, g.ldk = B, H, W, self.cp, self.kh, self.kw, self.stride, self.pad, self.cout, self.ldk
        return g

    def forward(self, lib, x, B, H, W, T16, wk, want_stats=True):
        """x: [B*H*W, cp] 16-bit, wk: the packed weight [cout, ldk] -> (y [B*Ho*Wo, cout] 16-bit, BatchNorm partials
        [2][cout][ceil(M/128)] or None, Ho, Wo).  Implicit GEMM (mh_conv_fwd): no im2col panel; the epilogue leaves the
        per-tile column sums BatchNorm needs."""
        Ho, Wo = self.out_hw(H, W)
        M = B * Ho * Wo
        y = torch.empty((M, self.cout), dtype=T16, device=x.device)
        part = torch.empty((2, self.cout, (M + 127) // 128), dtype=F32, device=x.device) if want_stats else None
        geom = self.geom(B, H, W)
        if self.grouped:
            check(lib.mh_gconv_fwd(x.data_ptr(), wk.data_ptr(), y.data_ptr(), None if part is None else part.data_ptr(), geom, self.groups,
                                   _stream()), "mh_gconv_fwd")
            return y, part, Ho, Wo
        sp = int(lib.mh_conv_splitk(geom, 0))          # > 1: a few-tile, long-contraction layer is cut into K chunks (f32 slabs)
        ws = torch.empty((sp, M, self.cout), dtype=F32, device=x.device) if sp > 1 else None
        check(lib.mh_conv_fwd(x.data_ptr(), wk.data_ptr(), y.data_ptr(), None if part is None else part.data_ptr(),
                              None if ws is None else ws.data_ptr(), geom, _stream()), "mh_conv_fwd")
        return y, part, Ho, Wo

    def _wgrad_split(self, lib, M, target):
        tiles = ((self.cout + 127) // 128) * ((self.kh * self.kw * self.cp + 127) // 128)
        want = max(1, min(64, -(-target // tiles), M // 256))
        return max(1, lib.mh_gemm_ksplit_for(int(M), int(want)))

    def _grouped_backward(self, lib, dy, x, wk, B, H, W, gscale, grads, need_dx, below, pair):
        """The grouped route: the weight gradient straight into _grad_target (the nn.Conv2d layout, f32: no slabs, no finishing job), the
        input gradient by mh_gconv_dgrad."""
        if below is not None or pair is not None:
            raise _lib.MemehipError(f"the {GROUPED} input gradient has no BatchNorm epilogue and does not pair")
        geom = self.geom(B, H, W)
        g, acc = _grad_target(self.mod.weight, grads)
        ws = torch.empty(int(lib.mh_gconv_wgrad_workspace_elems(geom, self.groups)), dtype=F32, device=dy.device)
        check(lib.mh_gconv_wgrad(dy.data_ptr(), x.data_ptr(), g.data_ptr(), ws.data_ptr(), int(acc), 1.0 / gscale, geom, self.groups, _stream()),
              "mh_gconv_wgrad")
        if not need_dx:
            return None, None
        dx = torch.empty((B * H * W, self.cp), dtype=dy.dtype, device=dy.device)
        check(lib.mh_gconv_dgrad(dy.data_ptr(), wk.data_ptr(), dx.data_ptr(), geom, self.groups, _stream()), "mh_gconv_dgrad")
        return dx, None

    def backward(self, lib, dy, x, wk, B, H, W, Ho, Wo, gscale, wjobs, opts, need_dx=True, wq=None, below=None, addend=None, y_mask=None,
                 pair=None, grads=None):
        """dy [M, cout] 16-bit -> (dx [B*H*W, cp] 16-bit or None, the statistics partials of `below` or None).  The weight gradient
        (implicit GEMM over x, mh_conv_wgrad) is deferred into `wq` (flush_wgrads) or launched here; its split-K slabs are queued in
        `wjobs` (summed, un-packed and added to .grad for all convolutions at once at the end of the backward).  The input gradient
        goes by dgrad_route.  `below` (implicit route only: epilogue_takes_bn): the tape record whose BatchNorm (+ReLU) produced x
        -- the epilogue masks dx for it and sums its statistics, after adding `addend` and by the sign of `y_mask` if that is given.
        `pair` (pairs_with): (ds, dy2, wk2) -- the 1x1 / 2 downsample that reads the same x, its dy and packed weight: dx is the sum of both
        input gradients, from one mh_conv_dgrad_pair launch."""
        M, dev = B * Ho * Wo, dy.device
        if self.grouped:
            return self._grouped_backward(lib, dy, x, wk, B, H, W, gscale, grads, need_dx, below, pair)
        if wq is not None:
            wq.append((self, dy, x, B, H, W, Ho, Wo))
        else:
            sp = self._wgrad_split(lib, M, WGRAD_TILES)
            slabs = torch.empty((sp, self.cout, self.ldk), dtype=F32, device=dev)
            check(lib.mh_conv_wgrad(dy.data_ptr(), x.data_ptr(), slabs.data_ptr(), sp, 1.0 / gscale, self.geom(B, H, W), _stream()), "mh_conv_wgrad")
            wjobs.append((self, slabs, sp, dy, x))
        if not need_dx:
            return None, None
        route = dgrad_route(self, H, W, opts)
        if below is not None and route != IMPLICIT:
            raise _lib.MemehipError(f"the {route} input gradient has no BatchNorm epilogue")
        if pair is not None and not pairs_with(self, pair[0], H, W, opts):
            raise _lib.MemehipError("these two convolutions' input gradients do not pair")
        dx = torch.empty((B * H * W, self.cp), dtype=dy.dtype, device=dev)
        if route == IMPLICIT:
            geom = self.geom(B, H, W)
            sp = int(lib.mh_conv_splitk(geom, 1))
            ws = torch.empty((sp, B * H * W, self.cp), dtype=F32, device=dev) if sp > 1 else None
            fuse, part = None, None
            if below is not None:
                nblk = (B * H * W + 127) // 128 if self.stride == 1 else 4 * ((B * (H // 2) * (W // 2) + 127) // 128)
                part = torch.empty((2, self.cp, nblk), dtype=F32, device=dev)
                fuse = _bn_epilogue(below, part, addend=addend, y_mask=y_mask)
            if pair is not None:
                ds, dy2, wk2 = pair
                check(lib.mh_conv_dgrad_pair(dy.data_ptr(), wk.data_ptr(), dy2.data_ptr(), wk2.data_ptr(), ds.ldk, ds.cout, dx.data_ptr(), geom, fuse,
                                             _stream()), "mh_conv_dgrad_pair")
                return dx, part
            check(lib.mh_conv_dgrad(dy.data_ptr(), wk.data_ptr(), dx.data_ptr(), None if ws is None else ws.data_ptr(), geom, fuse, _stream()),
                  "mh_conv_dgrad")
            return dx, part
        dA = dx if route == GEMM else torch.empty((M, self.ldk), dtype=dy.dtype, device=dev)      # (GEMM: ldk == cp, the panel IS dx)
        if self.cout % 64 == 0:
            ops.gemm_grouped([ops.Gemm(dy, wk, dA, M, self.ldk, self.cout, self.cout, self.ldk, self.ldk)], False, True)
        else:
            # a contraction (= cout) that is no multiple of the 64-deep K tile: dy's rows are cout long, so the GEMM's K tile would run into the
            # next row (it refuses).  The panel dA = dy . wk IS a 1x1 convolution of dy ([B][Ho][Wo][cout]) with wk transposed, and mh_conv_fwd's
            # generic walk zero-fills a K tile past the last channel: the same 128x128 MFMA tile, no new kernel.  (wk^T: <= 36 KiB, made here.)
            kt = (self.cout + 63) // 64 * 64
            wt = torch.zeros((self.ldk, kt), dtype=dy.dtype, device=dev)
            wt[:, :self.cout] = wk.t()
            g = _lib.MhConvGeom()
            g.B, g.H, g.W, g.C, g.KH, g.KW, g.stride, g.pad, g.Cout, g.ldk = B, Ho, Wo, self.cout, 1, 1, 1, 0, self.ldk, kt
            check(lib.mh_conv_fwd(dy.data_ptr(), wt.data_ptr(), dA.data_ptr(), None, None, g, _stream()), "mh_conv_fwd (dgrad panel)")
        if route == COL2IM:
            check(lib.mh_col2im_nhwc(dA.data_ptr(), dx.data_ptr(), B, H, W, self.cp, self.kh, self.kw, self.stride, self.pad, self.ldk,
                                     _stream()), "mh_col2im_nhwc")
        return dx, None


def flush_wgrads(lib, wq, wjobs, gscale):
    """The deferred weight gradients of up to MH_CONV_MAX_GROUP convolutions as ONE launch (mh_conv_wgrad_grouped): alone each is
    ~256 tiles -- half of the 512 workgroup slots for ~26 us, most of it fill / epilogue; together they fill the slots with fewer K
    chunks (= fewer f32 slabs to write and sum) each."""
    if not wq:
        return
    n = len(wq)
    probs = (_lib.MhConvWgradProblem * n)()
    target = max(48, 512 // n)
    for i, (cv, dy, x, B, H, W, Ho, Wo) in enumerate(wq):
        M = B * Ho * Wo
        sp = cv._wgrad_split(lib, M, target)
        slabs = torch.empty((sp, cv.cout, cv.ldk), dtype=F32, device=dy.device)
        probs[i].dy, probs[i].x, probs[i].slabs = dy.data_ptr(), x.data_ptr(), slabs.data_ptr()
        probs[i].ksplit, probs[i].alpha, probs[i].geom = sp, 1.0 / gscale, cv.geom(B, H, W)
        wjobs.append((cv, slabs, sp, dy, x))
    check(lib.mh_conv_wgrad_grouped(probs, n, _stream()), "mh_conv_wgrad_grouped")
    wq.clear()


class _BN:
    def __init__(self, mod: nn.BatchNorm2d):
        self.mod = mod
        self.C = mod.num_features

    def _ws(self, M, dev):
        return torch.empty(int(_lib.load().mh_bn2d_workspace_elems(M, self.C)), dtype=F32, device=dev)

    def forward(self, lib, x, M, residual, relu, training, part=None):
        m = self.mod
        y = torch.empty_like(x)
        sm, sr = torch.empty(self.C, dtype=F32, device=x.device), torch.empty(self.C, dtype=F32, device=x.device)
        res, momentum = None if residual is None else residual.data_ptr(), float(m.momentum if m.momentum is not None else 0.1)
        if training and part is not None:      # batch statistics from the convolution epilogue's per-tile sums: no pass over x
            check(lib.mh_bn2d_fwd_parts(x.data_ptr(), part.data_ptr(), part.shape[2], m.weight.data_ptr(), m.bias.data_ptr(),
                                        m.running_mean.data_ptr(), m.running_var.data_ptr(), res, y.data_ptr(), sm.data_ptr(), sr.data_ptr(),
                                        M, self.C, float(m.eps), momentum, int(relu), _stream()), "mh_bn2d_fwd_parts")
            return y, sm, sr
        ws = self._ws(M, x.device)
        check(lib.mh_bn2d_fwd(x.data_ptr(), m.weight.data_ptr(), m.bias.data_ptr(), m.running_mean.data_ptr(), m.running_var.data_ptr(),
                              res, y.data_ptr(), sm.data_ptr(), sr.data_ptr(), ws.data_ptr(), M, self.C, float(m.eps), momentum,
                              int(training), int(relu), _stream()), "mh_bn2d_fwd")
        return y, sm, sr

    def _param_grad_targets(self, grads):
        """(dgamma, dbeta, accumulate): where the two parameter gradients go (_grad_target), as one in-place / fresh decision"""
        m = self.mod
        dg, acc_g = _grad_target(m.weight, grads)
        db, acc_b = _grad_target(m.bias, grads)
        if acc_g != acc_b:      # (one of the two has a usable .grad and the other does not: take the slow path for both)
            dg, db = torch.empty_like(m.weight), torch.empty_like(m.bias)
            grads[id(m.weight)], grads[id(m.bias)] = dg, db
            acc_g = False
        return dg, db, acc_g

    def backward(self, lib, dy, x, y, sm, sr, M, relu, want_dres, gscale, grads):
        m = self.mod
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if want_dres else None
        dg, db, acc = self._param_grad_targets(grads)
        ws = self._ws(M, x.device)
        flags = (_lib.MH_BN_RELU if relu else 0) | (_lib.MH_BN_ACCUM_PARAM_GRADS if acc else 0)
        check(lib.mh_bn2d_bwd(dy.data_ptr(), x.data_ptr(), None if y is None else y.data_ptr(), m.weight.data_ptr(), m.bias.data_ptr(), sm.data_ptr(),
                              sr.data_ptr(), dx.data_ptr(), None if dres is None else dres.data_ptr(), dg.data_ptr(), db.data_ptr(),
                              ws.data_ptr(), M, self.C, flags, 1.0 / gscale, _stream()), "mh_bn2d_bwd")
        return dx, dres

    def backward_parts(self, lib, dy_masked, x, sm, sr, part, M, gscale, grads):
        """BatchNorm2d backward when the producing dgrad epilogue already masked dy and summed its statistics (mh_conv_dgrad with `below`)."""
        dx = torch.empty_like(x)
        dg, db, acc = self._param_grad_targets(grads)
        sums = torch.empty((2, self.C), dtype=F32, device=x.device)
        check(lib.mh_bn2d_bwd_parts(dy_masked.data_ptr(), x.data_ptr(), part.data_ptr(), part.shape[2], self.mod.weight.data_ptr(), sm.data_ptr(),
                                    sr.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), sums.data_ptr(), M, self.C,
                                    _lib.MH_BN_ACCUM_PARAM_GRADS if acc else 0, 1.0 / gscale, _stream()), "mh_bn2d_bwd_parts")
        return dx


@dataclass
class ConvBnRec:
    """One conv + BatchNorm (+ residual) (+ ReLU), y = act(bn(z = conv(x)) [+ residual]).  `conv` and `bn` alone: the layer's launch objects, built
    once per model (ResNet50._units), shared by the forward, the weight pack and the backward; every field: what one forward left on the tape."""
    conv: _Conv
    bn: _BN
    x: torch.Tensor = None         # [B*H*W, cp] 16-bit input
    wk: torch.Tensor = None        # packed weight [cout, ldk]
    z: torch.Tensor = None         # conv output = BatchNorm input [B*Ho*Wo, cout]
    y: torch.Tensor = None
    mean: torch.Tensor = None      # the statistics the forward normalised with
    rstd: torch.Tensor = None
    H: int = 0                     # input and output size
    W: int = 0
    Ho: int = 0
    Wo: int = 0
    relu: bool = True
    has_res: bool = False          # a residual was added before the ReLU


@dataclass
class SERec:
    """A block's squeeze-and-excitation gate: `mod` alone is the parameter holder (_ConvTower._block_units); every field: what one forward left
    on the tape.  out = relu(u * s + shortcut) with u the y of the chain's last record (bn3: no residual, no ReLU)."""
    mod: "SEModule"
    pooled: torch.Tensor = None    # [B, C] f32, mean_hw u
    hidden: torch.Tensor = None    # [B, R] f32, after the ReLU
    s: torch.Tensor = None         # [B, C] f32, the gate
    out: torch.Tensor = None       # [B*Ho*Wo, C] 16-bit, the block's output


@dataclass
class BlockRec:
    """One residual block's layers (bottleneck: conv1-3; basic block: conv1-2) + downsample: _ResNet._block_units, and on the tape their
    records of one forward.  `chain`: the main branch in order; its last unit takes the residual and the block's ReLU -- unless the block
    has a squeeze-and-excitation gate (`se`): then the last unit stores bn3 alone and the gate's `out` is the block's output."""
    conv1: ConvBnRec
    conv2: ConvBnRec
    conv3: Optional[ConvBnRec] = None
    downsample: Optional[ConvBnRec] = None
    se: Optional[SERec] = None

    @property
    def chain(self) -> List[ConvBnRec]:
        return [u for u in (self.conv1, self.conv2, self.conv3) if u is not None]

    @property
    def units(self) -> List[ConvBnRec]:
        return self.chain + ([] if self.downsample is None else [self.downsample])


@dataclass
class PoolRec:
    arg: torch.Tensor        # uint8 index of the maximum in its window
    H: int
    W: int
    C: int


@dataclass
class Tape:
    B: int
    stem: ConvBnRec
    pool: PoolRec
    blocks: List[BlockRec]
    pooled: torch.Tensor
    last_hw: tuple
    dtype: torch.dtype


def se_reduced_channels(channels: int) -> int:
    """timm's ``make_divisible(channels / 16, 8, round_limit=0.)``, the hidden width of a ResNet block's SEModule: 16 / 32 / 64 / 128 for
    256 / 512 / 1024 / 2048 channels"""
    return max(8, int(channels / 16 + 4) // 8 * 8)


class SEModule(nn.Module):
    """timm.layers.SEModule (``fc1``: Conv2d(C, R, 1) -> ReLU -> ``fc2``: Conv2d(R, C, 1) -> sigmoid, both with bias; its ``bn`` / ``act`` /
    ``gate`` members hold no state): parameter holder, the arithmetic is mh_se_*."""

    def __init__(self, channels: int, rd_channels: int):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, rd_channels, 1, bias=True)
        self.fc2 = nn.Conv2d(rd_channels, channels, 1, bias=True)


class Bottleneck(nn.Module):
    """torchvision.models.resnet.Bottleneck (v1.5: the stride sits on the 3x3 convolution): parameter holder.  ``groups`` / ``base_width``:
    ResNeXt's grouped conv2 over ``width = int(planes * base_width / 64) * groups`` channels.  ``se``: timm's ``attn_layer='se'`` -- a member
    ``se`` (SEModule) between bn3 and the residual add; without it the module has no such member."""
    expansion = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: bool = False, groups: int = 1, base_width: int = 64,
                 se: bool = False):
        super().__init__()
        width = int(planes * base_width / 64) * groups      # torchvision's rule; the defaults give width = planes (ResNet-50)
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        if se:
            self.se = SEModule(planes * 4, se_reduced_channels(planes * 4))
        self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4)) if downsample else None
        self.stride = stride

    def conv_bn_pairs(self):
        """(the main branch's (conv, bn) in order, the shortcut's or None): what _ConvTower._wire reads of a block"""
        return [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)], (None if self.downsample is None else tuple(self.downsample))


class BasicBlock(nn.Module):
    """torchvision.models.resnet.BasicBlock (= timm's for resnet18 / 34): parameter holder."""
    expansion = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: bool = False):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride=stride, bias=False), nn.BatchNorm2d(planes)) if downsample else None
        self.stride = stride

    def conv_bn_pairs(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2)], (None if self.downsample is None else tuple(self.downsample))


class _TowerFn(torch.autograd.Function):
    """Opaque autograd node: the whole conv tower forward; backward walks the saved tape."""

    @staticmethod
    def forward(ctx, image, net, *params):
        ctx.net = net
        ctx.tape = net._forward_tape(image, training=net.training)
        return ctx.tape.pooled.clone()

    @staticmethod
    def backward(ctx, d_pooled):
        grads = ctx.net._backward_tape(ctx.tape, d_pooled)
        ctx.tape = None
        return (None, None) + tuple(grads[id(p)] for p in ctx.net._tower_params)


def stage_blocks(stages, make_block):
    """The blocks of a residual tower from its stage list [(blocks, in, out, stride)], one list per stage: a stage's first block takes the
    stride and the channel change, and a projection shortcut when either is there; ``make_block(cin, cout, stride, shortcut)`` builds the
    parameter holder under its family's names (torchvision's ``layerN.i.convK`` / transformers' ``stages.N.layers.i.layer.K``)."""
    return [[make_block(cin if bi == 0 else cout, cout, stride if bi == 0 else 1, bi == 0 and (stride != 1 or cin != cout)) for bi in range(n)]
            for n, cin, cout, stride in stages]


class _ConvTower(nn.Module):
    """A stem (7x7 / 2 conv + BatchNorm + ReLU + 3x3 / 2 max pool), residual blocks, global average pool on the HIP kernels: the ONE
    forward and backward walk of every ResNet family here.  A subclass builds its parameter holders under its own names and hands them to
    ``_wire``; ``features(image f32 [B, in_channels, H, W])`` returns the pooled ``feature_dim`` features; ``options``: the backward's
    TowerOptions."""

    def _init_tower(self, compute_dtype: str, grad_stream_scale: float, options: TowerOptions):
        if compute_dtype not in ("bf16", "fp16"):
            raise ValueError(f"compute_dtype must be 'bf16' or 'fp16', got {compute_dtype!r}")
        self.compute_dtype = compute_dtype
        self.options = options
        self.gscale = float(grad_stream_scale) if grad_stream_scale else (8192.0 if compute_dtype == "fp16" else 1.0)

    def _wire(self, stem_conv: nn.Conv2d, stem_bn: nn.BatchNorm2d, blocks, tower_params: List[nn.Parameter]):
        """`blocks`: the holders in forward order (each with ``conv_bn_pairs()``); the stem's input channels are zero-padded to 8."""
        self._tower_params = tower_params

        def unit(conv, bn, cin_pad=None):
            return ConvBnRec(_Conv(conv, cin_pad), _BN(bn))
        self.in_channels = stem_conv.in_channels
        self._stem_unit = unit(stem_conv, stem_bn, 8)
        self._block_units = []
        for b in blocks:
            chain, shortcut = b.conv_bn_pairs()
            c = [unit(*cb) for cb in chain]
            se = getattr(b, "se", None)
            self._block_units.append(BlockRec(c[0], c[1], c[2] if len(c) > 2 else None, None if shortcut is None else unit(*shortcut),
                                              None if se is None else SERec(se)))
        self._units = [self._stem_unit] + [u for b in self._block_units for u in b.units]
        self.feature_dim = self._block_units[-1].chain[-1].conv.cout

    # ---- launches ----------------------------------------------------------------------------------------------
    def _forward_tape(self, image: torch.Tensor, training: bool) -> Tape:
        if not image.is_cuda:
            raise _lib.MemehipError(f"{type(self).__name__} runs on the HIP device only (no CPU fallback): move the batch with .to(device)")
        lib = _lib.load(self.compute_dtype)
        T16 = torch.float16 if self.compute_dtype == "fp16" else torch.bfloat16
        B, Cc, H, W = image.shape
        if Cc != self.in_channels:
            raise ValueError(f"{type(self).__name__} expects {self.in_channels}-channel images")
        x = torch.empty((B * H * W, 8), dtype=T16, device=image.device)
        img32 = image.to(F32).contiguous()      # named: a temporary would be freed (and its block re-used) before the launch
        check(lib.mh_nchw_to_nhwc(img32.data_ptr(), x.data_ptr(), B, Cc, H, W, 8, _stream()), "mh_nchw_to_nhwc")
        packed = self._pack_all_weights(lib, T16)
        def conv_bn(u, xin, h, w, residual=None, relu=True) -> ConvBnRec:
            wk = packed[id(u.conv.mod)]
            z, part, ho, wo = u.conv.forward(lib, xin, B, h, w, T16, wk, want_stats=training)
            y, sm, sr = u.bn.forward(lib, z, B * ho * wo, residual, relu, training, part)
            return ConvBnRec(u.conv, u.bn, xin, wk, z, y, sm, sr, h, w, ho, wo, relu, residual is not None)

        stem = conv_bn(self._stem_unit, x, H, W)
        C1 = self._stem_unit.conv.cout
        h, w = (stem.Ho + 2 - 3) // 2 + 1, (stem.Wo + 2 - 3) // 2 + 1
        x = torch.empty((B * h * w, C1), dtype=T16, device=image.device)
        arg = torch.empty((B * h * w, C1), dtype=torch.uint8, device=image.device)
        check(lib.mh_maxpool_fwd(stem.y.data_ptr(), x.data_ptr(), arg.data_ptr(), B, stem.Ho, stem.Wo, C1, 3, 2, 1, _stream()), "mh_maxpool_fwd")
        blocks = []
        for u in self._block_units:      # one rule for both block types: the chain but its last unit, the downsample, the last unit + residual
            *body, last = u.chain
            recs, y, hh, ww = [], x, h, w
            for v in body:
                recs.append(conv_bn(v, y, hh, ww))
                y, hh, ww = recs[-1].y, recs[-1].Ho, recs[-1].Wo
            ds = None if u.downsample is None else conv_bn(u.downsample, x, h, w, relu=False)
            shortcut, se = (x if ds is None else ds.y), None
            if u.se is None:
                recs.append(conv_bn(last, y, hh, ww, residual=shortcut, relu=True))
            else:      # squeeze-and-excitation: bn3 alone, then the gate and out = relu(u * s + shortcut)
                recs.append(conv_bn(last, y, hh, ww, residual=None, relu=False))
                se = self._se_forward(lib, u.se.mod, recs[-1], shortcut, B)
            blocks.append(BlockRec(*recs, downsample=ds, se=se))
            x, h, w = (recs[-1].y if se is None else se.out), recs[-1].Ho, recs[-1].Wo
        pooled = torch.empty((B, self.feature_dim), dtype=F32, device=image.device)
        check(lib.mh_avgpool_fwd(x.data_ptr(), pooled.data_ptr(), B, h * w, self.feature_dim, _stream()), "mh_avgpool_fwd")
        if training:      # nn.BatchNorm2d's step counter, all of them (53 in ResNet-50) in one multi-tensor launch
            torch._foreach_add_([u.bn.mod.num_batches_tracked for u in self._units], 1)
        return Tape(B, stem, PoolRec(arg, stem.Ho, stem.Wo, C1), blocks, pooled, (h, w), T16)

    @staticmethod
    def _se_forward(lib, mod, rec: ConvBnRec, shortcut: torch.Tensor, B: int) -> SERec:
        """The gate of one SE block over u = rec.y [B*HW, C]: squeeze (the global average pool), excite, scale + shortcut + ReLU."""
        u, HW, C, R = rec.y, rec.Ho * rec.Wo, mod.fc1.in_channels, mod.fc1.out_channels
        pooled, s = torch.empty((B, C), dtype=F32, device=u.device), torch.empty((B, C), dtype=F32, device=u.device)
        hidden, out = torch.empty((B, R), dtype=F32, device=u.device), torch.empty_like(u)
        check(lib.mh_avgpool_fwd(u.data_ptr(), pooled.data_ptr(), B, HW, C, _stream()), "mh_avgpool_fwd")
        check(lib.mh_se_gate_fwd(pooled.data_ptr(), mod.fc1.weight.data_ptr(), mod.fc1.bias.data_ptr(), mod.fc2.weight.data_ptr(),
                                 mod.fc2.bias.data_ptr(), hidden.data_ptr(), s.data_ptr(), B, C, R, _stream()), "mh_se_gate_fwd")
        check(lib.mh_se_apply_fwd(u.data_ptr(), s.data_ptr(), shortcut.data_ptr(), out.data_ptr(), B, HW, C, _stream()), "mh_se_apply_fwd")
        return SERec(mod, pooled, hidden, s, out)

    def _se_backward(self, lib, se: SERec, rec: ConvBnRec, dy: torch.Tensor, B: int, grads: dict):
        """dy: the FULL gradient of an SE block's output -> (du, the gradient of u = rec.y; g, the gradient of the shortcut branch)."""
        mod, HW, (_, C), R = se.mod, rec.Ho * rec.Wo, se.s.shape, se.hidden.shape[1]
        g, du = torch.empty_like(dy), torch.empty_like(dy)
        ds, dpooled = torch.empty_like(se.s), torch.empty_like(se.s)
        check(lib.mh_se_apply_bwd_reduce(dy.data_ptr(), se.out.data_ptr(), rec.y.data_ptr(), g.data_ptr(), ds.data_ptr(), B, HW, C, _stream()),
              "mh_se_apply_bwd_reduce")
        (dw1, db1, dw2, db2), acc = _grad_targets([mod.fc1.weight, mod.fc1.bias, mod.fc2.weight, mod.fc2.bias], grads)
        check(lib.mh_se_gate_bwd(ds.data_ptr(), se.s.data_ptr(), se.hidden.data_ptr(), se.pooled.data_ptr(), mod.fc1.weight.data_ptr(),
                                 mod.fc2.weight.data_ptr(), dpooled.data_ptr(), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(),
                                 B, C, R, 1.0 / self.gscale, int(acc), _stream()), "mh_se_gate_bwd")
        check(lib.mh_se_apply_bwd(g.data_ptr(), se.s.data_ptr(), dpooled.data_ptr(), du.data_ptr(), B, HW, C, _stream()), "mh_se_apply_bwd")
        return du, g

    def _convs(self):
        """(conv module, input channels of its NHWC activation) in a fixed order"""
        return [(u.conv.mod, u.conv.cp) for u in self._units]

    def _pack_all_weights(self, lib, T16):
        """f32 [Cout][Cin][kh][kw] -> 16-bit [Cout][(kh,kw,c)] for every convolution: one buffer, mh_conv_weight_pack_batched
        launches of <= 64 jobs."""
        convs = [u.conv for u in self._units if not u.conv.grouped]
        total = sum(c.cout * c.ldk for c in convs)
        dev = self._stem_unit.conv.mod.weight.device
        buf = torch.empty(total, dtype=T16, device=dev)
        packed, off = {}, 0
        for c in (u.conv for u in self._units if u.conv.grouped):      # the grouped route's own fragment images
            wk = torch.empty(int(lib.mh_gconv_packed_elems(c.cout, c.groups)), dtype=T16, device=dev)
            check(lib.mh_gconv_weight_pack(c.mod.weight.data_ptr(), wk.data_ptr(), c.cout, c.groups, _stream()), "mh_gconv_weight_pack")
            packed[id(c.mod)] = wk
        for i in range(0, len(convs), _lib.MH_CONV_MAX_JOBS):
            chunk = convs[i:i + _lib.MH_CONV_MAX_JOBS]
            jobs = (_lib.MhConvPackJob * len(chunk))()
            for j, c in enumerate(chunk):
                wk = buf[off:off + c.cout * c.ldk].view(c.cout, c.ldk)
                off += c.cout * c.ldk
                packed[id(c.mod)] = wk
                jobs[j].w, jobs[j].out = c.mod.weight.data_ptr(), wk.data_ptr()
                jobs[j].Cout, jobs[j].Cin, jobs[j].KH, jobs[j].KW, jobs[j].Cp, jobs[j].ldk = c.cout, c.cin, c.kh, c.kw, c.cp, c.ldk
            check(lib.mh_conv_weight_pack_batched(jobs, len(chunk), _stream()), "mh_conv_weight_pack_batched")
        return packed

    def _backward_tape(self, tape: Tape, d_pooled: torch.Tensor):
        lib, opts = _lib.load(self.compute_dtype), self.options
        B, T16, (h, w), Cf, dev = tape.B, tape.dtype, tape.last_hw, self.feature_dim, d_pooled.device
        dx = torch.empty((B * h * w, Cf), dtype=T16, device=dev)
        dp32 = d_pooled.to(F32).contiguous()
        check(lib.mh_avgpool_bwd(dp32.data_ptr(), dx.data_ptr(), B, h * w, Cf, self.gscale, _stream()), "mh_avgpool_bwd")
        grads = {}      # id(parameter) -> gradient tensor for autograd, or None when it was accumulated into .grad in place
        wjobs = []      # (conv, split-K slabs of its weight gradient, nsplit, operands kept alive): finished in one launch at the end
        group = max(1, min(opts.wgrad_group, _lib.MH_CONV_MAX_GROUP))
        wq = [] if group > 1 else None

        def conv_bn_bwd(rec, dy, want_dres=False, need_dx=True, pre_part=None, below=None, block_out=False, addend=None, pair=None):
            """Backward of one conv + BatchNorm (+ReLU) -> (dx, the residual branch's gradient, statistics partials of `below`, dz).
            `pre_part`: dy arrives MASKED with its column sums already taken by the dgrad epilogue that produced it.  `below`: the
            record whose output is this convolution's input -- when its BatchNorm has a ReLU and no residual, this dgrad's epilogue
            does that BatchNorm's masking and statistics (epilogue_takes_bn).  `block_out` (+ `addend`): the block_out form, `pair`
            (a downsample's record and its dz): the two input gradients in one launch; see the block loop."""
            M = B * rec.Ho * rec.Wo
            if pre_part is not None:
                dz = rec.bn.backward_parts(lib, dy, rec.z, rec.mean, rec.rstd, pre_part, M, self.gscale, grads)
                dres = dy if want_dres else None          # the masked gradient IS the gradient of the residual branch
            else:
                # the ReLU mask: from y where a residual was added before the ReLU, recomputed from z otherwise (one tensor less to read)
                dz, dres = rec.bn.backward(lib, dy, rec.z, rec.y if (rec.relu and rec.has_res) else None, rec.mean, rec.rstd, M, rec.relu,
                                           want_dres, self.gscale, grads)
            if not block_out and not (below is not None and below.relu and not below.has_res
                                      and epilogue_takes_bn(rec.conv, rec.H, rec.W, opts)):
                below = None
            dxin, part = rec.conv.backward(lib, dz, rec.x, rec.wk, B, rec.H, rec.W, rec.Ho, rec.Wo, self.gscale, wjobs, opts, need_dx,
                                           wq=wq, below=below, addend=addend, y_mask=below.y if block_out else None,
                                           pair=None if pair is None else (pair[0].conv, pair[1], pair[0].wk), grads=grads)
            if wq is not None and len(wq) >= group:
                flush_wgrads(lib, wq, wjobs, self.gscale)
            return dxin, dres, part, dz

        dx_part = None       # statistics partials of the gradient in `dx` when a block's conv1 epilogue already masked it for the bn3 below
        for k in reversed(range(len(tape.blocks))):
            blk, below = tape.blocks[k], (tape.blocks[k - 1] if k else None)
            # One rule for both block types.  The chain's last unit (bn3 / bn2 + residual + relu): d_ident is the gradient of the identity branch;
            # every unit's dgrad epilogue already does the masking + statistics of the BatchNorm below it in the chain
            *body, last = blk.chain
            c1, ds = blk.conv1, blk.downsample
            if blk.se is None:
                d_o, d_ident, part, _ = conv_bn_bwd(last, dx, want_dres=True, below=body[-1], pre_part=dx_part)
            else:      # the gate first (dx is the full gradient of the block's output: see below_se), then bn3 with no mask and no residual
                du, d_ident = self._se_backward(lib, blk.se, last, dx, B, grads)
                d_o, _, part, _ = conv_bn_bwd(last, du, below=body[-1])
            # a basic block's 3x3 / 2 conv1 next to the 1x1 / 2 downsample: both read the block input -- the downsample leaves only its dz here,
            # its input gradient is a second K segment of conv1's dgrad (mh_conv_dgrad_pair)
            pair = None
            if ds is not None:
                paired = pairs_with(c1.conv, ds.conv, c1.H, c1.W, opts)
                d_ident, _, _, dz_ds = conv_bn_bwd(ds, d_ident, need_dx=not paired)      # downsample conv + bn (no relu)
                pair = (ds, dz_ds) if paired else None
            for j in range(len(body) - 1, 0, -1):
                d_o, _, part, _ = conv_bn_bwd(body[j], d_o, below=body[j - 1], pre_part=part)
            if below is not None and epilogue_takes_bn(c1.conv, c1.H, c1.W, opts, block_out=True, below_se=below.se is not None):
                # conv1's input is the output y = relu(bn(z) + residual) of the block below: its dgrad epilogue adds the gradient arriving
                # through the other branch (d_ident; paired: already in the accumulators), masks by y > 0 and takes that BatchNorm's statistics
                # -- no mh_add_h16 pass, no statistics pass (round 4)
                dx, _, dx_part, _ = conv_bn_bwd(c1, d_o, pre_part=part, below=below.chain[-1], block_out=True, addend=d_ident, pair=pair)
            elif pair is not None:
                dx, _, _, _ = conv_bn_bwd(c1, d_o, pre_part=part, pair=pair)
                dx_part = None
            else:
                d_o, _, _, _ = conv_bn_bwd(c1, d_o, pre_part=part)
                dx, dx_part = torch.empty_like(d_o), None
                check(lib.mh_add_h16(d_o.data_ptr(), d_ident.data_ptr(), dx.data_ptr(), d_o.numel(), _stream()), "mh_add_h16")
        pool = tape.pool
        dxp = torch.empty((B * pool.H * pool.W, pool.C), dtype=T16, device=dev)
        check(lib.mh_maxpool_bwd(dx.data_ptr(), pool.arg.data_ptr(), dxp.data_ptr(), B, pool.H, pool.W, pool.C, 3, 2, 1, _stream()), "mh_maxpool_bwd")
        conv_bn_bwd(tape.stem, dxp, need_dx=False)
        if wq:
            flush_wgrads(lib, wq, wjobs, self.gscale)
        for i0 in range(0, len(wjobs), _lib.MH_CONV_MAX_JOBS):
            chunk = wjobs[i0:i0 + _lib.MH_CONV_MAX_JOBS]
            jobs = (_lib.MhConvWgradJob * len(chunk))()
            for j, (cv, slabs, sp, _dy, _A) in enumerate(chunk):
                g, acc = _grad_target(cv.mod.weight, grads)
                jobs[j].slabs, jobs[j].g = slabs.data_ptr(), g.data_ptr()
                jobs[j].Cout, jobs[j].Cin, jobs[j].KH, jobs[j].KW, jobs[j].Cp, jobs[j].ldk = cv.cout, cv.cin, cv.kh, cv.kw, cv.cp, cv.ldk
                jobs[j].nsplit, jobs[j].accumulate, jobs[j].scale = sp, int(acc), 1.0
            check(lib.mh_conv_wgrad_finish_batched(jobs, len(chunk), _stream()), "mh_conv_wgrad_finish_batched")
        return grads

    # ---- nn.Module surface ------------------------------------------------------------------------------------------
    def features(self, image: torch.Tensor) -> torch.Tensor:
        if torch.is_grad_enabled() and self.training:
            return _TowerFn.apply(image, self, *self._tower_params)
        return self._forward_tape(image, training=self.training).pooled


class _ResNet(_ConvTower):
    """torchvision ResNet topology and state_dict over one block type (`block`: Bottleneck / BasicBlock) on the HIP kernels.
    ``forward(image f32 [B,3,H,W]) -> logits [B, num_classes]`` (``num_classes=0``: no classifier, the features, as timm's
    ``reset_classifier(0)``); ``features(image)`` returns the pooled ``feature_dim`` features;
    ``options``: the backward's TowerOptions."""
    block = None
    default_layers = None
    groups, width_per_group = 1, 64      # (Bottleneck only: ResNeXt)
    se = False                           # (Bottleneck only: a squeeze-and-excitation gate in every block)

    def __init__(self, num_classes: int = 1000, compute_dtype: str = "fp16", layers=None, width: int = 64,
                 grad_stream_scale: float = 0.0, seed: int = 0, options: TowerOptions = TowerOptions()):
        super().__init__()
        block, layers = self.block, (self.default_layers if layers is None else layers)
        self._init_tower(compute_dtype, grad_stream_scale, options)
        torch.manual_seed(seed)
        self.conv1 = nn.Conv2d(3, width, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        outs = [width * m * block.expansion for m in (1, 2, 4, 8)]
        stages = list(zip(layers, [width] + outs[:-1], outs, (1, 2, 2, 2)))      # (blocks, in, out, stride); four `layerN` at the most
        extra = dict(groups=self.groups, base_width=self.width_per_group) if self.groups > 1 else {}
        se_kw = dict(se=True) if self.se else {}
        for _, _, cout, _ in stages if extra else ():
            cg = int(cout // block.expansion * self.width_per_group / 64)
            if cg not in (4, 8, 16, 32):
                raise ValueError(f"{type(self).__name__}: width={width} gives grouped convolutions of {cg} channels per group; the kernels have 4, 8, 16 and 32")
        built = stage_blocks(stages, lambda cin, cout, stride, shortcut: block(cin, cout // block.expansion, stride, downsample=shortcut, **extra, **se_kw))
        for li, blocks in enumerate(built, 1):
            setattr(self, f"layer{li}", nn.Sequential(*blocks))
        inplanes = stages[-1][2]
        self.fc = nn.Linear(inplanes, num_classes) if num_classes > 0 else nn.Identity()      # 0: timm's reset_classifier(0), forward = features
        for m in self.modules():          # torchvision's initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        self._wire(self.conv1, self.bn1, [b for blocks in built for b in blocks],
                   [p for n, p in self.named_parameters() if not n.startswith("fc.")])

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        f = self.features(image)
        return f if isinstance(self.fc, nn.Identity) else fused.linear(f, self.fc.weight, self.fc.bias)


class ResNet50(_ResNet):
    """torchvision ``resnet50``: bottleneck blocks (3, 4, 6, 3), 2048-d features."""
    block, default_layers = Bottleneck, (3, 4, 6, 3)


class ResNet18(_ResNet):
    """torchvision / timm ``resnet18``: basic blocks (2, 2, 2, 2), 512-d features (what ``reset_classifier(0)`` leaves)."""
    block, default_layers = BasicBlock, (2, 2, 2, 2)


class ResNet34(_ResNet):
    """torchvision / timm ``resnet34``: basic blocks (3, 4, 6, 3), 512-d features."""
    block, default_layers = BasicBlock, (3, 4, 6, 3)


class ResNeXt50_32x4d(_ResNet):
    """torchvision ``resnext50_32x4d`` (Kevin's Subtask-2B image zoo, example_scripts/Untitled-2.py:210-237): ResNet-50's tree with every
    bottleneck's 3x3 a 32-group convolution over 128 / 256 / 512 / 1024 channels (4 / 8 / 16 / 32 per group), 2048-d features;
    25 028 904 parameters with the 1000-way ``fc``.  The grouped layers run on mh_gconv_* (csrc/groupconv.hip)."""
    block, default_layers = Bottleneck, (3, 4, 6, 3)
    groups, width_per_group = 32, 4


class SEResNeXt50_32x4d(_ResNet):
    """timm ``seresnext50_32x4d`` (the first model of Kevin's Subtask-2B image zoo, example_scripts/Untitled-2.py:182-207): ``ResNeXt50_32x4d``
    with a squeeze-and-excitation gate (``layerN.i.se.fc1 / fc2``, hidden width 16 / 32 / 64 / 128) in every bottleneck; 27 559 896 parameters
    with the 1000-way ``fc``.  Every other key is torchvision's, as for the ResNeXt tower.  The gates run on mh_se_* (csrc/se.hip)."""
    block, default_layers = Bottleneck, (3, 4, 6, 3)
    groups, width_per_group = 32, 4
    se = True


RESNETS = {"resnet50": ResNet50, "resnet18": ResNet18, "resnet34": ResNet34, "resnext50_32x4d": ResNeXt50_32x4d,
           "seresnext50_32x4d": SEResNeXt50_32x4d}


# ---- transformers' ResNet (models/resnet/modeling_resnet.py): the same network under transformers' module names ----------------------
class HFConvLayer(nn.Module):
    """transformers' ResNetConvLayer / ResNetShortCut: ``convolution`` + ``normalization`` (the activation has no state): parameter holder."""

    def __init__(self, cin: int, cout: int, kernel_size: int = 3, stride: int = 1):
        super().__init__()
        self.convolution = nn.Conv2d(cin, cout, kernel_size, stride=stride, padding=kernel_size // 2, bias=False)
        self.normalization = nn.BatchNorm2d(cout)


class HFLayer(nn.Module):
    """transformers' ResNetBasicLayer (3x3, 3x3) / ResNetBottleNeckLayer (1x1 to out / 4, 3x3 with the stride, 1x1): ``shortcut`` (a
    projection, or nn.Identity) and ``layer`` (the main branch): parameter holder."""

    def __init__(self, cin: int, cout: int, stride: int, shortcut: bool, bottleneck: bool):
        super().__init__()
        self.shortcut = HFConvLayer(cin, cout, 1, stride) if shortcut else nn.Identity()
        mid = cout // 4
        self.layer = nn.Sequential(HFConvLayer(cin, mid, 1), HFConvLayer(mid, mid, 3, stride), HFConvLayer(mid, cout, 1)) if bottleneck else \
            nn.Sequential(HFConvLayer(cin, cout, 3, stride), HFConvLayer(cout, cout, 3))

    def conv_bn_pairs(self):
        s = self.shortcut
        return [(u.convolution, u.normalization) for u in self.layer], (None if isinstance(s, nn.Identity) else (s.convolution, s.normalization))


class HFStage(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.layers = nn.Sequential(*layers)


class HFEmbeddings(nn.Module):
    def __init__(self, num_channels: int, embedding_size: int):
        super().__init__()
        self.embedder = HFConvLayer(num_channels, embedding_size, 7, 2)
        self.pooler = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)


class HFEncoder(nn.Module):
    def __init__(self, stages):
        super().__init__()
        self.stages = nn.ModuleList(stages)


HF_RESNET_DEFAULTS = dict(num_channels=3, embedding_size=64, hidden_sizes=(256, 512, 1024, 2048), depths=(3, 4, 6, 3), layer_type="bottleneck",
                          hidden_act="relu", downsample_in_first_stage=False, downsample_in_bottleneck=False, num_labels=2)


class HFResNetModel(_ConvTower):
    """transformers' ``ResNetModel`` (``embedder.embedder.convolution``, ``encoder.stages.N.layers.i.shortcut / layer.K`` ...) on the tower
    walk: ``forward(pixel_values)`` returns the pooled features [B, hidden_sizes[-1]]."""

    def __init__(self, cfg: dict, compute_dtype: str, grad_stream_scale: float, options: TowerOptions):
        super().__init__()
        self._init_tower(compute_dtype, grad_stream_scale, options)
        hidden, depths = list(cfg["hidden_sizes"]), list(cfg["depths"])
        bottleneck = cfg["layer_type"] == "bottleneck"
        self.embedder = HFEmbeddings(cfg["num_channels"], cfg["embedding_size"])
        stages = list(zip(depths, [cfg["embedding_size"]] + hidden[:-1], hidden, [2 if cfg["downsample_in_first_stage"] else 1] + [2] * (len(hidden) - 1)))
        built = stage_blocks(stages, lambda cin, cout, stride, shortcut: HFLayer(cin, cout, stride, shortcut, bottleneck))
        self.encoder = HFEncoder([HFStage(layers) for layers in built])
        self.pooler = nn.AdaptiveAvgPool2d((1, 1))
        for m in self.modules():          # transformers' ResNetPreTrainedModel._init_weights
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        self._wire(self.embedder.embedder.convolution, self.embedder.embedder.normalization, [b for layers in built for b in layers],
                   list(self.parameters()))

    def forward(self, pixel_values: torch.Tensor) -> torch.Tensor:
        return self.features(pixel_values)


class HFResNetForImageClassification(nn.Module):
    """transformers' ``ResNetForImageClassification`` as the organizers' Subtask-2B example builds it (ResNet_example_task2B.py:146-167:
    ``ResNetConfig(num_channels=1, layer_type="basic", depths=[2, 2], hidden_sizes=[32, 64], num_labels=...)``) on the HIP tower:
    transformers' module tree and state_dict, key for key (``resnet.encoder.stages.0.layers.0.shortcut.convolution.weight``,
    ``classifier.1.bias``, every ``num_batches_tracked``), so ``load_state_dict`` takes the library model's weights and the Hub's HF-format
    ResNet checkpoints (``microsoft/resnet-18`` / ``-50``) and gives them back.  ``config``: a ``transformers.ResNetConfig`` (or any object
    / dict with its fields), or the fields as keywords with ResNetConfig's defaults.  Every channel count (for bottleneck layers
    ``hidden // 4`` too) must be a multiple of 8; ``hidden_act != "relu"`` and ``downsample_in_bottleneck=True`` are refused.
    ``model(pixel_values=..., labels=...)`` -> ``(loss, logits)``; without labels ``logits`` (HF Trainer's protocol)."""

    def __init__(self, config=None, compute_dtype: str = "fp16", grad_stream_scale: float = 0.0, seed: int = 0,
                 options: TowerOptions = TowerOptions(), **fields):
        super().__init__()
        unknown = sorted(set(fields) - set(HF_RESNET_DEFAULTS))
        if unknown:
            raise TypeError(f"HFResNetForImageClassification: unknown configuration fields {unknown}")
        get = (lambda k, d: config.get(k, d)) if isinstance(config, dict) else (lambda k, d: getattr(config, k, d))
        cfg = {k: fields[k] if k in fields else (d if config is None else get(k, d)) for k, d in HF_RESNET_DEFAULTS.items()}
        if cfg["hidden_act"] != "relu":
            raise ValueError(f"hidden_act must be 'relu' (the kernels fuse the ReLU), got {cfg['hidden_act']!r}")
        if cfg["downsample_in_bottleneck"]:
            raise ValueError("downsample_in_bottleneck=True is not supported (the stride sits on the 3x3 convolution)")
        if cfg["layer_type"] not in ("basic", "bottleneck"):
            raise ValueError(f"layer_type must be 'basic' or 'bottleneck', got {cfg['layer_type']!r}")
        if cfg["num_channels"] not in (1, 3):
            raise ValueError(f"num_channels must be 1 or 3, got {cfg['num_channels']!r}")
        hidden, depths = list(cfg["hidden_sizes"]), list(cfg["depths"])
        if not 1 <= len(hidden) <= 4 or len(depths) != len(hidden) or min(depths) < 1:
            raise ValueError(f"hidden_sizes and depths must name the same 1 to 4 stages of at least one layer, got {hidden} and {depths}")
        if cfg["embedding_size"] < 8 or cfg["embedding_size"] % 8:
            raise ValueError(f"embedding_size must be a multiple of 8 (the kernels' channel granule), got {cfg['embedding_size']}")
        for h in hidden:
            if h < 8 or h % 8:
                raise ValueError(f"hidden_sizes must be multiples of 8 (the kernels' channel granule), got {hidden}")
            if cfg["layer_type"] == "bottleneck" and (h // 4 < 8 or (h // 4) % 8 or h % 4):
                raise ValueError(f"hidden_sizes of bottleneck layers must be multiples of 32 (hidden // 4 a multiple of 8), got {hidden}")
        if int(cfg["num_labels"]) < 1:
            raise ValueError(f"num_labels must be positive, got {cfg['num_labels']!r}")
        self.resnet_config = cfg          # (a dict, and not named `config`: transformers.Trainer writes its own fields into a model's .config)
        self.num_labels = int(cfg["num_labels"])
        torch.manual_seed(seed)
        self.resnet = HFResNetModel(cfg, compute_dtype, grad_stream_scale, options)
        self.classifier = nn.Sequential(nn.Flatten(), nn.Linear(hidden[-1], self.num_labels))
        self.loss_fct = CrossEntropyLoss()

    def forward(self, pixel_values=None, labels=None, **unused):
        if pixel_values is None:
            raise ValueError("HFResNetForImageClassification.forward needs pixel_values")
        fc = self.classifier[1]
        logits = fused.linear(self.resnet(pixel_values), fc.weight, fc.bias)
        if labels is not None:
            return self.loss_fct(logits, labels.view(-1)), logits
        return logits


class ResNetClassifier(nn.Module):
    """The ResNet-50 surface of BASELINE config 2 under the Subtask-2B Trainer protocol (ResNet_example_task2B.py:206-221):
    ``model(pixel_values=..., labels=...)`` -> ``(loss, logits)``; without labels ``logits``.  ``arch``: "resnet50" (default) | "resnet18" |
    "resnet34" | "resnext50_32x4d" | "seresnext50_32x4d", torchvision's keys (+ timm's ``se.*``).  The model the 2B example itself builds (a ``ResNetConfig``) is ``HFResNetForImageClassification``."""

    def __init__(self, num_labels: int = 2, compute_dtype: str = "fp16", arch: str = "resnet50", **kw):
        super().__init__()
        if arch not in RESNETS:
            raise ValueError(f"arch must be one of {sorted(RESNETS)}, got {arch!r}")
        self.resnet = RESNETS[arch](num_classes=num_labels, compute_dtype=compute_dtype, **kw)
        self.loss_fct = CrossEntropyLoss()

    def forward(self, pixel_values=None, labels=None, **unused):
        if pixel_values is None:
            raise ValueError("ResNetClassifier.forward needs pixel_values")
        logits = self.resnet(pixel_values)
        if labels is not None:
            return self.loss_fct(logits, labels.view(-1)), logits
        return logits
