"""ResNeXt-50 32x4d on the MI355X.

Part A -- the grouped 3x3 kernels alone (mh_gconv_packed_elems / mh_gconv_weight_pack / mh_gconv_fwd / mh_gconv_dgrad /
  mh_gconv_wgrad_workspace_elems / mh_gconv_wgrad) against ``F.conv2d(..., groups=...)`` and its autograd in float64 on the CPU:
  exact on integer operands (bit for bit, BatchNorm partials included), no leakage between groups, random operands inside the bound of
  an f32 sum taken in any order (2^-p |ref| for the one output rounding + n 2^-24 sum|terms|), a weight gradient that is the same bits
  on every call, and refusals that write nothing.  The small cases give every weight-gradient workgroup ONE unit of 32 pixels; the
  ``walk_*`` cases give it two or three, as every grouped layer of the benchmarked tower does (batch 32, 224 px: 2 to 13), so the loop's
  prefetch, its closing barrier and the accumulators carried across units run here with a ragged last chunk -- for every Cg at both
  strides, all three unit shapes, C = 288 (four bundles and a half, Cg = 32 included), an odd x even stride-2 image and several forward /
  dgrad tiles.  The regime is read from the library (workspace / (C Cg 9) = chunks, against the unit count of every unit shape), not
  restated; a guard walks the real tower and asserts that every (Cg, stride, walks) it launches is among the cases; and a batch split
  in two accumulating launches (other chunk boundaries) must give the bits of the one launch.
Part B -- ``ResNeXt50_32x4d(layers=(1, 1, 1, 1))`` forward + backward against the float64 composition of
  tests/test_basic_resnet_gpu.py part B extended to bottlenecks with groups: the same 16-bit storage points (straight-through), the
  same bars.  Then gradient accumulation, the classifier under the fused Adam, Kevin's three-tower model and ``ResNeXt50_32x4d_BH``
  (with mh_l2norm_fwd / mh_l2norm_bwd alone) over the new tower."""
import importlib.util
import os
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from conftest import parity_log

pytestmark = pytest.mark.gpu
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("T16", [F16, BF16], ids=["fp16", "bf16"])
HALF_ULP = {F16: 2.0 ** -11, BF16: 2.0 ** -8}          # half an ulp of the one output rounding, relative
MH_EINVAL, MH_ESHAPE = 1, 2

# (B, H, W, C, groups, stride)
CASES = {
    "cg4_odd": (2, 7, 5, 32, 8, 1),            # Cg = 4, one 32-channel bundle, odd non-square
    "cg8_odd_s2": (2, 7, 5, 64, 8, 2),         # Cg = 8, two bundles, odd size with stride 2
    "pixel_s1": (1, 1, 1, 64, 4, 1),           # a single pixel: every tap but the centre is padding
    "pixel_s2": (1, 1, 1, 64, 4, 2),
    "cg16_s2": (2, 3, 3, 32, 2, 2),            # Cg = 16
    "cg32_two_tiles": (3, 9, 9, 64, 2, 1),     # Cg = 32, 243 rows: a second, partial 128-row tile for bn_part
    "layer1_s2": (2, 8, 8, 128, 32, 2),        # the first ResNeXt layer's own grouping
    # beyond the issue's list: one wide row, where the weight gradient takes its 1 x 32 unit shape (every case above takes 2 x 16 or 4 x 8);
    # every case down to here: one unit per workgroup
    "wide_s1": (1, 1, 40, 32, 8, 1),
    "wide_s2": (1, 2, 80, 32, 8, 2),
    # The walk: more units than workgroups asked for (512 / bundles), so a workgroup loops over `per` >= 2 units and the last chunk is
    # ragged -- the only way the benchmarked tower runs this kernel.  unit, per, chunks (units): what the plan gives today; the test pins
    # only chunks < units of every unit shape (test_gconv_cases_pin_their_walk_regime).
    #                                                  Cg, stride   unit   per  chunks (units)   further edge
    "walk_cg4_s1": (7, 17, 17, 288, 72, 1),          #  4, 1        4 x 8   2   53 (105)   C = 288: four bundles + half a bundle; 16 forward tiles
    "walk_cg8_s2": (7, 17, 66, 288, 36, 2),          #  8, 2        4 x 8   2   53 (105)   odd x even image; 62 dgrad tiles
    "walk_cg16_s1": (7, 5, 66, 288, 18, 1),          # 16, 1        2 x 16  2   53 (105)   2 x 16 with the Cg <= 16 body
    "walk_cg32_s2": (7, 9, 130, 288, 9, 2),          # 32, 2        2 x 16  2   53 (105)   <true, 2>, <9, *> at stride 2, half a bundle with Cg = 32
    "walk_cg32_s1": (7, 17, 17, 288, 9, 1),          # 32, 1        4 x 8   2   53 (105)   loads issued at the top of each unit (the Cg = 32 route)
    "walk_row_cg4_s1": (3, 1, 733, 512, 128, 1),     #  4, 1        1 x 32  2   35 (69)    a one-row image, ragged last segment
    "walk_row_cg32_s2": (3, 1, 660, 1024, 32, 2),    # 32, 2        1 x 32  2   17 (33)    the 195-pixel halo, the largest one
    "walk_three": (10, 13, 16, 1024, 256, 1),        #  4, 1        2 x 16  3   24 (70)    three units per workgroup, the last chunk one
    # the two (Cg, stride) pairs of the real tower (layer2's later blocks, layer3's first) that the eight above leave out:
    # test_gconv_cases_cover_what_the_benchmarked_tower_launches asks for them
    "walk_cg8_s1": (7, 17, 17, 288, 36, 1),          #  8, 1        4 x 8   2   53 (105)
    "walk_cg16_s2": (7, 9, 130, 288, 18, 2),         # 16, 2        2 x 16  2   53 (105)   2 x 16 at stride 2 with the Cg <= 16 body (7 halo chunks prefetched)
    # the one stride-2 image parity left (odd x odd, even x even and odd x even are above): even x odd, one unit per workgroup
    "cg8_even_odd_s2": (2, 6, 9, 64, 8, 2),
}
OLD_CASES = [c for c in CASES if not c.startswith("walk_")]
WALK_CASES = [c for c in CASES if c.startswith("walk_")]
CASE = pytest.mark.parametrize("case", list(CASES))
UNIT_SHAPES = ((4, 8), (2, 16), (1, 32))          # rows x columns of the 32 output pixels of a weight-gradient unit


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import multimodal_propaganda_meme_classification_amd as m
    return m


def _lib(pkg, T16):
    return pkg._lib.load("fp16" if T16 == F16 else "bf16")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _name(T16):
    return "fp16" if T16 == F16 else "bf16"


def _nhwc(x4):
    return x4.permute(0, 2, 3, 1).reshape(-1, x4.shape[1]).contiguous()


def _geom(pkg, B, H, W, C, stride, k=3, pad=1, cout=None):
    g = pkg._lib.MhConvGeom()
    g.B, g.H, g.W, g.C, g.KH, g.KW, g.stride, g.pad, g.Cout, g.ldk = B, H, W, C, k, k, stride, pad, C if cout is None else cout, 0
    return g


def _out(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def _conv_refs(x, w, dy, groups, stride):
    """float64: y, dx, dw of F.conv2d(groups=...) -- y and dx as NHWC matrices"""
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=stride, padding=1, groups=groups)
    y.backward(dy)
    return _nhwc(y.detach()), _nhwc(xr.grad), wr.grad


class _Run:
    """the device side of one case: operands (float64 tensors holding 16-bit values) -> the four launches; the batch is x's (the case's, or a
    part of it)"""

    def __init__(self, pkg, T16, case, x, w, dy):
        self.pkg, self.lib, self.T16 = pkg, _lib(pkg, T16), T16
        _, self.H, self.W, self.C, self.groups, self.stride = CASES[case]
        self.B = x.shape[0]
        assert x.shape[1:] == (self.C, self.H, self.W) and dy.shape[0] == self.B
        self.Ho, self.Wo = _out(self.H, self.W, self.stride)
        self.M, self.Mi = self.B * self.Ho * self.Wo, self.B * self.H * self.W
        self.geom = _geom(pkg, self.B, self.H, self.W, self.C, self.stride)
        self.x = _nhwc(x).to(T16).cuda()
        self.dy = _nhwc(dy).to(T16).cuda()
        self.w32 = w.to(F32).cuda().contiguous()
        n = int(self.lib.mh_gconv_packed_elems(self.C, self.groups))
        assert n == 2 * (self.C // 16) * (9 if self.C // self.groups == 32 else 5) * 512
        self.wk = torch.full((n + 64,), 7.0, dtype=T16, device="cuda")
        pkg._lib.check(self.lib.mh_gconv_weight_pack(self.w32.data_ptr(), self.wk.data_ptr(), self.C, self.groups, _st()), "mh_gconv_weight_pack")
        torch.cuda.synchronize()
        assert bool((self.wk[n:] == 7.0).all()), "the pack wrote past wk"

    def fwd(self, stats=True):
        nblk = (self.M + 127) // 128
        y = torch.full((self.M + 16, self.C), 7.0, dtype=self.T16, device="cuda")
        part = torch.full((2 * self.C * nblk + 64,), 12345.0, dtype=F32, device="cuda")
        self.pkg._lib.check(self.lib.mh_gconv_fwd(self.x.data_ptr(), self.wk.data_ptr(), y.data_ptr(), part.data_ptr() if stats else None, self.geom,
                                                  self.groups, _st()), "mh_gconv_fwd")
        torch.cuda.synchronize()
        assert bool((y[self.M:] == 7.0).all()) and bool((part[2 * self.C * nblk:] == 12345.0).all()), "mh_gconv_fwd wrote past its outputs"
        if not stats:
            assert bool((part == 12345.0).all())
        return y[:self.M].cpu(), part[:2 * self.C * nblk].view(2, self.C, nblk).cpu()

    def dgrad(self):
        dx = torch.full((self.Mi + 16, self.C), 7.0, dtype=self.T16, device="cuda")
        self.pkg._lib.check(self.lib.mh_gconv_dgrad(self.dy.data_ptr(), self.wk.data_ptr(), dx.data_ptr(), self.geom, self.groups, _st()), "mh_gconv_dgrad")
        torch.cuda.synchronize()
        assert bool((dx[self.Mi:] == 7.0).all()), "mh_gconv_dgrad wrote past dx"
        return dx[:self.Mi].cpu()

    def workspace(self):
        n = int(self.lib.mh_gconv_wgrad_workspace_elems(self.geom, self.groups))
        assert n > 0 and n % (self.C * (self.C // self.groups) * 9) == 0
        return n, torch.full((n + 64,), float("nan"), dtype=F32, device="cuda")

    def wgrad(self, ws=None, dw=None, accumulate=0, alpha=1.0):
        n, fresh = self.workspace()
        ws = fresh if ws is None else ws
        if dw is None:
            dw = torch.full((self.C * (self.C // self.groups) * 9 + 64,), 12345.0, dtype=F32, device="cuda")
        self.pkg._lib.check(self.lib.mh_gconv_wgrad(self.dy.data_ptr(), self.x.data_ptr(), dw.data_ptr(), ws.data_ptr(), accumulate, alpha, self.geom,
                                                    self.groups, _st()), "mh_gconv_wgrad")
        torch.cuda.synchronize()
        nd = self.C * (self.C // self.groups) * 9
        assert bool((dw[nd:] == 12345.0).all()), "mh_gconv_wgrad wrote past dw"
        assert bool(torch.isnan(ws[n:]).all()) or ws.numel() == n, "mh_gconv_wgrad wrote past its workspace"
        return dw[:nd].view(self.C, self.C // self.groups, 3, 3).cpu()


@lru_cache(maxsize=None)
def _integer_operands(case):
    B, H, W, C, groups, stride = CASES[case]
    Ho, Wo = _out(H, W, stride)
    g = torch.Generator().manual_seed(300 + list(CASES).index(case))
    ri = lambda shape, a: torch.randint(-a, a + 1, shape, generator=g).to(F64)
    x, w, dy = ri((B, C, H, W), 4), ri((C, C // groups, 3, 3), 2), ri((B, C, Ho, Wo), 3)
    assert not torch.equal(w, w.transpose(2, 3)) and (C // groups < 2 or not torch.equal(w[:C // groups], w[:C // groups].transpose(0, 1)))
    return (x, w, dy) + _conv_refs(x, w, dy, groups, stride)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _chunks(pkg, lib, B, H, W, C, groups, stride):
    """the weight gradient's workgroups per 64-channel bundle, from the host-only workspace query: one [C][Cg][9] f32 partial each"""
    n = int(lib.mh_gconv_wgrad_workspace_elems(_geom(pkg, B, H, W, C, stride), groups))
    assert n > 0 and n % (C * (C // groups) * 9) == 0
    return n // (C * (C // groups) * 9)


def _unit_counts(B, H, W, stride):
    """how many units of 32 output pixels the batch has under each unit shape"""
    Ho, Wo = _out(H, W, stride)
    return [B * -(-Ho // rt) * -(-Wo // wt) for rt, wt in UNIT_SHAPES]


def _walks(pkg, lib, B, H, W, C, groups, stride):
    """fewer workgroups than units under EVERY unit shape: whichever shape the plan chose, some workgroup loops over two units or more"""
    return _chunks(pkg, lib, B, H, W, C, groups, stride) < min(_unit_counts(B, H, W, stride))


@CASE
def test_gconv_cases_pin_their_walk_regime(pkg, case):
    """No launch: the plan is host code.  The small cases are the one-unit regime (as many workgroups as units of some shape), every
    walk_* case has fewer workgroups than units of any shape, walk_three fewer than half as many."""
    B, H, W, C, groups, stride = CASES[case]
    assert B * H * W * C <= 2_500_000
    for T16 in (F16, BF16):
        chunks, units = _chunks(pkg, _lib(pkg, T16), *CASES[case]), _unit_counts(B, H, W, stride)
        if case in OLD_CASES:
            assert chunks in units, f"{chunks} workgroups, units per shape {units}: no longer one unit per workgroup"
        else:
            assert chunks < min(units), f"{chunks} workgroups, units per shape {units}: no workgroup has to walk"
        if case == "walk_three":
            assert 2 * chunks < min(units), f"{chunks} workgroups, units per shape {units}: no workgroup walks three units"


def _tower_grouped_launches(pkg, batch, size):
    """(B, H, W, C, groups, stride) of every grouped convolution of ResNeXt-50 32x4d on `size` x `size` images, walked as
    _ConvTower._forward_tape walks (stem, max pool, each block's chain) -- on the host, no launch"""
    net = pkg.ResNeXt50_32x4d(num_classes=2, compute_dtype="fp16")
    h, w = net._stem_unit.conv.out_hw(size, size)
    h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    out = []
    for blk in net._block_units:
        hh, ww = h, w
        for u in blk.chain:
            if u.conv.grouped:
                assert u.conv.cin == u.conv.cout
                out.append((batch, hh, ww, u.conv.cout, u.conv.groups, u.conv.stride))
            hh, ww = u.conv.out_hw(hh, ww)
        h, w = hh, ww
    return out


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BENCH_BATCH, BENCH_SIZE = 32, 224          # tools/resnext_bench.py's --batch / --image-size defaults: the measured ResNeXt step


def test_gconv_cases_cover_what_the_benchmarked_tower_launches(pkg):
    """No launch.  Every (Cg, stride, walks?) among the grouped layers of the real tower at the benchmark's batch and size occurs among
    CASES: a change of the workgroup cap or of the unit rule that moves production into a regime no exact test runs fails here (as does
    dropping the cases).  The layers come from the tower itself; tools/resnext_bench.py's table must be the same set."""
    lib = _lib(pkg, F16)
    launches = _tower_grouped_launches(pkg, BENCH_BATCH, BENCH_SIZE)
    assert len(launches) == 16          # one per bottleneck: 3 + 4 + 6 + 3
    shapes = set(launches)                # the distinct geometries: the stride-1 and the stride-2 block of each layer
    bench = _load_tool("resnext_bench")
    assert bench.GROUPS == 32 and sorted((C, HW, st) for _, C, HW, st in bench.LAYERS) == sorted((C, H, st) for _, H, _, C, _, st in shapes)
    assert len(shapes) == 7 and all(g == 32 for *_, g, _ in shapes)          # (layer1's two kinds of block are one geometry: no stride there)
    have = set()
    for c, (B, H, W, C, g, st) in CASES.items():
        walks = _walks(pkg, lib, B, H, W, C, g, st)
        assert walks == (c in WALK_CASES), f"{c}: walks = {walks}, against its name (test_gconv_cases_pin_their_walk_regime)"
        have.add((C // g, st, walks))
    want = {(C // g, st, _walks(pkg, lib, B, H, W, C, g, st)): (B, H, W, C, g, st) for B, H, W, C, g, st in shapes}
    missing = {k: v for k, v in want.items() if k not in have}
    assert not missing, f"(Cg, stride, walks) of the benchmarked tower that no case of CASES runs: {missing}"


@DTYPES
@CASE
def test_gconv_is_exact_on_integers(pkg, case, T16):
    """|x| <= 4, |w| <= 2, |dy| <= 3: every product and every partial sum is an integer below 2^24 (forward / dgrad: <= 9 * 32 * 8; wgrad:
    <= 12 M, M <= 2275 output pixels), exact in f32 in any order -- y and dx are the float64 result rounded once, dw is the float64 result,
    bn_part the sums of the stored values per 128-row tile and column (integers; the test asserts their y^2 sums stay below 2^24 too).
    In the walk_* cases dw is the sum over the two or three units each workgroup walked: an accumulator reset per unit, a unit staged from
    the wrong registers or read while the next one is being written changes integers."""
    x, w, dy, y_ref, dx_ref, dw_ref = _integer_operands(case)
    r = _Run(pkg, T16, case, x, w, dy)
    y, part = r.fwd()
    want = y_ref.to(T16)
    assert torch.equal(_bits(y), _bits(want)), f"forward: {int((y != want).sum())} of {y.numel()} elements differ"
    tile = torch.arange(r.M) // 128
    ys = want.to(F64)
    s1 = torch.zeros((part.shape[2], r.C), dtype=F64).index_add_(0, tile, ys)
    s2 = torch.zeros((part.shape[2], r.C), dtype=F64).index_add_(0, tile, ys * ys)
    assert float(s2.max()) < 2 ** 24
    assert torch.equal(part[0].to(F64), s1.t()) and torch.equal(part[1].to(F64), s2.t()), "bn_part is not the per-tile sums of the stored y, y^2"
    y2, _ = r.fwd(stats=False)
    assert torch.equal(_bits(y2), _bits(want))
    dx = r.dgrad()
    assert torch.equal(_bits(dx), _bits(dx_ref.to(T16))), f"dgrad: {int((dx != dx_ref.to(T16)).sum())} of {dx.numel()} elements differ"
    dw = r.wgrad()
    assert float(dw_ref.abs().max()) < 2 ** 24
    assert torch.equal(dw.to(F64), dw_ref), f"wgrad: {int((dw.to(F64) != dw_ref).sum())} of {dw.numel()} elements differ"


# the live groups of a case, beyond the rule's one (group 2, or the last of fewer than four): walk_cg4_s1 -- group 70 = channels 280..283,
# inside the half-empty last bundle (256..287), beside group 2 in a full one; walk_cg32_s2 -- group 8 = channels 256..287, that half bundle
LEAK_GROUPS = {"walk_cg4_s1": (70,), "walk_cg32_s2": (8,)}


@DTYPES
@pytest.mark.parametrize("case", ["cg4_odd", "cg8_odd_s2", "cg16_s2", "cg32_two_tiles", "layer1_s2", "walk_cg16_s1", "walk_cg32_s2", "walk_cg4_s1"])
def test_gconv_does_not_leak_between_groups(pkg, case, T16):
    B, H, W, C, groups, stride = CASES[case]
    Ho, Wo = _out(H, W, stride)
    cg = C // groups
    for grp in (groups - 1 if groups < 4 else 2,) + LEAK_GROUPS.get(case, ()):
        g = torch.Generator().manual_seed(41)
        w = torch.randint(1, 3, (C, cg, 3, 3), generator=g).to(F64)          # no zero weight: a leak cannot hide
        x, dy = torch.zeros((B, C, H, W), dtype=F64), torch.zeros((B, C, Ho, Wo), dtype=F64)
        x[:, grp * cg:(grp + 1) * cg] = torch.randint(1, 5, (B, cg, H, W), generator=g).to(F64)
        dy[:, grp * cg:(grp + 1) * cg] = torch.randint(1, 4, (B, cg, Ho, Wo), generator=g).to(F64)
        r = _Run(pkg, T16, case, x, w, dy)
        y, _ = r.fwd()
        dx = r.dgrad()
        inside = torch.zeros(C, dtype=torch.bool)
        inside[grp * cg:(grp + 1) * cg] = True
        assert bool((y[:, ~inside] == 0).all()), f"group {grp}: y is nonzero outside the one group that has input"
        assert bool((dx[:, ~inside] == 0).all()), f"group {grp}: dx is nonzero outside the one group that has a gradient"
        assert bool((y[:, inside] > 0).all()) and bool((dx[:, inside] > 0).all()), f"group {grp}"
        dw = r.wgrad()                                                        # (H, W >= 3 in these cases: every tap meets a pixel)
        assert bool((dw[~inside] == 0).all()), f"group {grp}: dw is nonzero in filters whose outputs have no gradient"
        assert bool((dw[inside] > 0).all()), f"group {grp}"


@lru_cache(maxsize=None)
def _random_operands(case, T16):
    B, H, W, C, groups, stride = CASES[case]
    Ho, Wo = _out(H, W, stride)
    g = torch.Generator().manual_seed(500 + 2 * list(CASES).index(case) + (T16 == BF16))
    rn = lambda shape: torch.randn(shape, generator=g, dtype=F64).to(T16).to(F64)
    x, w, dy = rn((B, C, H, W)), rn((C, C // groups, 3, 3)), rn((B, C, Ho, Wo))
    return (x, w, dy), _conv_refs(x, w, dy, groups, stride), _conv_refs(x.abs(), w.abs(), dy.abs(), groups, stride)


@DTYPES
@CASE
def test_gconv_random_operands_within_the_f32_sum_bound(pkg, case, T16):
    """|got - ref| <= 2^-p |ref| + n 2^-24 A element by element: half an ulp of the one output rounding (p = 11 fp16, 8 bf16; none for the
    f32 weight gradient) plus the bound of an n-term f32 sum in any order, A = the same convolution of the absolute values."""
    (x, w, dy), (y_ref, dx_ref, dw_ref), (y_abs, dx_abs, dw_abs) = _random_operands(case, T16)
    r = _Run(pkg, T16, case, x, w, dy)
    cg = r.C // r.groups
    y, _ = r.fwd()
    dx, dw = r.dgrad(), r.wgrad()
    worst = {}
    for what, got, ref, A, n, half in (("fwd", y, y_ref, y_abs, 9 * cg, HALF_ULP[T16]), ("dgrad", dx, dx_ref, dx_abs, 9 * cg, HALF_ULP[T16]),
                                       ("wgrad", dw, dw_ref, dw_abs, r.M, 0.0)):
        got = got.to(F64)
        assert torch.isfinite(got).all(), what
        bar = half * ref.abs() + n * 2.0 ** -24 * A
        frac = ((got - ref).abs() / bar.clamp_min(1e-300)).max()
        worst[what] = float(frac)
        assert bool(((got - ref).abs() <= bar).all()), f"{what}: worst error {float(frac):.3g} x the bar"
    parity_log(f"[gconv {case} {_name(T16)}] worst error / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@DTYPES
@pytest.mark.parametrize("case", ["cg8_odd_s2", "cg32_two_tiles", "layer1_s2", "walk_cg8_s2", "walk_cg32_s1", "walk_three"])
def test_gconv_wgrad_is_deterministic_and_accumulates(pkg, case, T16):
    (x, w, dy), (_, _, dw_ref), _ = _random_operands(case, T16)
    r = _Run(pkg, T16, case, x, w, dy)
    n, ws = r.workspace()
    first = r.wgrad(ws=ws)
    second = r.wgrad(ws=ws)
    ws.normal_()                                   # an unrelated launch over the same workspace
    ws[n:] = float("nan")
    y, _ = r.fwd()
    third = r.wgrad(ws=ws)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32)) and torch.equal(first.view(torch.int32), third.view(torch.int32))
    # accumulate: prefill + the accumulate = 0 result, one f32 rounding per element
    g = torch.Generator().manual_seed(9)
    pre = torch.randn(first.numel() + 64, generator=g)
    dw = pre.clone().cuda()
    dw[first.numel():] = 12345.0
    acc = r.wgrad(ws=ws, dw=dw, accumulate=1)
    want = (pre[:first.numel()].view_as(first).to(F64) + first.to(F64))
    assert bool(((acc.to(F64) - want).abs() <= 2.0 ** -24 * want.abs() + 1e-45).all())
    half = r.wgrad(ws=ws, alpha=0.5)               # alpha scales the sum (a power of two: exactly)
    assert torch.equal(half, first * 0.5)


@DTYPES
@pytest.mark.parametrize("case", ["walk_cg8_s2", "walk_cg32_s2"])
def test_gconv_wgrad_walk_equals_a_split_batch(pkg, case, T16):
    """Integer operands, so every sum is exact whatever its order: the weight gradient of the 7 images in one launch, and that of images
    [0, 3) followed by that of [3, 7) with accumulate = 1 -- other unit counts, so other chunk boundaries (today the parts are small enough
    for one unit per workgroup: the walked sum against the unwalked one) -- are the same bits, those of the float64 reference."""
    x, w, dy, _, _, dw_ref = _integer_operands(case)
    B, H, W, C, groups, stride = CASES[case]
    assert B == 7
    whole = _Run(pkg, T16, case, x, w, dy)
    a, b = _Run(pkg, T16, case, x[:3], w, dy[:3]), _Run(pkg, T16, case, x[3:], w, dy[3:])
    lib = _lib(pkg, T16)
    assert _walks(pkg, lib, 7, H, W, C, groups, stride)
    assert _chunks(pkg, lib, 7, H, W, C, groups, stride) != _chunks(pkg, lib, 3, H, W, C, groups, stride) + _chunks(pkg, lib, 4, H, W, C, groups, stride)
    dw_whole = whole.wgrad()
    dw = torch.full((dw_ref.numel() + 64,), 12345.0, dtype=F32, device="cuda")
    first = a.wgrad(dw=dw)
    both = b.wgrad(dw=dw, accumulate=1)
    assert not torch.equal(first, both)
    assert torch.equal(dw_whole.view(torch.int32), both.view(torch.int32)), f"{int((dw_whole != both).sum())} of {both.numel()} elements differ"
    assert torch.equal(both.to(F64), dw_ref)


@DTYPES
def test_gconv_refusals_write_nothing(pkg, T16):
    lib = _lib(pkg, T16)
    B, H, W, C, groups = 2, 6, 6, 64, 8
    M = B * H * W
    mk = lambda *shape: torch.zeros(shape, dtype=T16, device="cuda")
    x, dy = mk(M + 8, C), mk(M + 8, C)
    wk = mk(int(lib.mh_gconv_packed_elems(C, groups)) + 8)
    y = torch.full((M + 8, C), 7.0, dtype=T16, device="cuda")
    part = torch.full((2, C, 1), 7.0, dtype=F32, device="cuda")
    dw = torch.full((C * 8 * 9 + 8,), 7.0, dtype=F32, device="cuda")
    ws = torch.full((int(lib.mh_gconv_wgrad_workspace_elems(_geom(pkg, B, H, W, C, 1), groups)) + 8,), 7.0, dtype=F32, device="cuda")
    w32 = torch.zeros((C, 8, 3, 3), device="cuda")
    wk_out = torch.full((wk.numel(),), 7.0, dtype=T16, device="cuda")
    good = dict(geom=(B, H, W, C, 1), groups=groups)

    def fwd(xp=x.data_ptr(), wkp=wk.data_ptr(), yp=y.data_ptr(), pp=part.data_ptr(), geom=good["geom"], groups=groups, **gk):
        return lib.mh_gconv_fwd(xp, wkp, yp, pp, _geom(pkg, *geom, **gk), groups, _st())

    def dgrad(dyp=dy.data_ptr(), wkp=wk.data_ptr(), dxp=y.data_ptr(), geom=good["geom"], groups=groups, **gk):
        return lib.mh_gconv_dgrad(dyp, wkp, dxp, _geom(pkg, *geom, **gk), groups, _st())

    def wgrad(dyp=dy.data_ptr(), xp=x.data_ptr(), dwp=dw.data_ptr(), wsp=ws.data_ptr(), geom=good["geom"], groups=groups, **gk):
        return lib.mh_gconv_wgrad(dyp, xp, dwp, wsp, 0, 1.0, _geom(pkg, *geom, **gk), groups, _st())

    shapes = {
        "Cg = 2": dict(groups=32), "Cg = 64": dict(geom=(B, H, W, 128, 1), groups=2), "C % 32": dict(geom=(B, H, W, 48, 1), groups=6),
        "5x5": dict(k=5, pad=2), "1x1": dict(k=1, pad=0), "pad 0": dict(pad=0), "stride 3": dict(geom=(B, H, W, C, 3)),
        "groups = 0": dict(groups=0), "Cout != C": dict(cout=128), "B = 0": dict(geom=(0, H, W, C, 1)),
    }
    got = {}
    for what, kw in shapes.items():
        got[what] = [(f(**kw), MH_ESHAPE) for f in (fwd, dgrad, wgrad)]
        g = _geom(pkg, *kw.get("geom", good["geom"]), **{k: v for k, v in kw.items() if k in ("k", "pad", "cout")})
        got[what].append((0 if int(lib.mh_gconv_wgrad_workspace_elems(g, kw.get("groups", groups))) == 0 else -1, 0))
    for what, (c, gr) in {"Cg = 2": (64, 32), "Cg = 64": (128, 2), "C % 32": (48, 6), "groups = 0": (64, 0)}.items():
        got["pack " + what] = [(lib.mh_gconv_weight_pack(w32.data_ptr(), wk_out.data_ptr(), c, gr, _st()), MH_ESHAPE),
                               (int(lib.mh_gconv_packed_elems(c, gr)), 0)]
    got["pointers"] = [
        (fwd(xp=None), MH_EINVAL), (fwd(wkp=None), MH_EINVAL), (fwd(yp=None), MH_EINVAL), (fwd(xp=x.data_ptr() + 2), MH_EINVAL),
        (fwd(wkp=wk.data_ptr() + 2), MH_EINVAL), (fwd(yp=y.data_ptr() + 2), MH_EINVAL), (fwd(pp=part.data_ptr() + 2), MH_EINVAL),
        (dgrad(dyp=None), MH_EINVAL), (dgrad(wkp=None), MH_EINVAL), (dgrad(dxp=None), MH_EINVAL), (dgrad(dyp=dy.data_ptr() + 2), MH_EINVAL),
        (dgrad(dxp=y.data_ptr() + 2), MH_EINVAL), (wgrad(dyp=None), MH_EINVAL), (wgrad(xp=None), MH_EINVAL), (wgrad(dwp=None), MH_EINVAL),
        (wgrad(wsp=None), MH_EINVAL), (wgrad(xp=x.data_ptr() + 2), MH_EINVAL), (wgrad(dwp=dw.data_ptr() + 2), MH_EINVAL),
        (lib.mh_gconv_weight_pack(None, wk_out.data_ptr(), C, groups, _st()), MH_EINVAL),
        (lib.mh_gconv_weight_pack(w32.data_ptr(), None, C, groups, _st()), MH_EINVAL),
        (lib.mh_gconv_weight_pack(w32.data_ptr(), wk_out.data_ptr() + 2, C, groups, _st()), MH_EINVAL),
    ]
    torch.cuda.synchronize()
    for what, pairs in got.items():
        for i, (status, want) in enumerate(pairs):
            assert status == want, f"{what} (call {i}): status {status}, expected {want}"
    for t in (y, part, dw, ws, wk_out):
        assert bool((t == 7.0).all()), "a refused call wrote to an output"
    # the same calls with complete, valid arguments
    assert lib.mh_gconv_weight_pack(w32.data_ptr(), wk_out.data_ptr(), C, groups, _st()) == 0
    assert fwd() == 0 and wgrad() == 0
    torch.cuda.synchronize()
    assert bool((y[:M] == 0).all()) and bool((y[M:] == 7.0).all()) and bool((part == 0).all()) and bool((dw[:C * 72] == 0).all())
    assert bool((wk_out[:-8] == 0).all()) and bool((wk_out[-8:] == 7.0).all())
    assert dgrad() == 0
    torch.cuda.synchronize()
    assert bool((y[:M] == 0).all()) and bool((y[M:] == 7.0).all())


def _l2norm_launch(pkg, x, g):
    """mh_l2norm_fwd + mh_l2norm_bwd over f32 [B, D] -> (y, norm, dx) on the CPU, nothing written past the outputs"""
    lib = pkg._lib.load()
    B, D = x.shape
    xd, gd = x.cuda(), g.cuda()
    y, norm, dx = torch.full((B * D + 64,), 7.0, device="cuda"), torch.full((B + 64,), 7.0, device="cuda"), torch.full((B * D + 64,), 7.0, device="cuda")
    pkg._lib.check(lib.mh_l2norm_fwd(xd.data_ptr(), y.data_ptr(), norm.data_ptr(), B, D, _st()), "mh_l2norm_fwd")
    pkg._lib.check(lib.mh_l2norm_bwd(gd.data_ptr(), y.data_ptr(), norm.data_ptr(), dx.data_ptr(), B, D, _st()), "mh_l2norm_bwd")
    torch.cuda.synchronize()
    assert bool((y[B * D:] == 7.0).all()) and bool((norm[B:] == 7.0).all()) and bool((dx[B * D:] == 7.0).all()), "mh_l2norm wrote past its outputs"
    assert lib.mh_l2norm_fwd(None, y.data_ptr(), norm.data_ptr(), B, D, _st()) == MH_EINVAL
    assert lib.mh_l2norm_bwd(gd.data_ptr(), y.data_ptr(), norm.data_ptr(), dx.data_ptr(), 0, D, _st()) == MH_ESHAPE
    return y[:B * D].view(B, D).cpu(), norm[:B].cpu(), dx[:B * D].view(B, D).cpu()


def _l2norm_misses(x, g, y, norm, dx, rows):
    """the bars of test_l2norm_against_float64 over `rows`: what misses them"""
    D = x.shape[1]
    x64 = x.to(F64).requires_grad_(True)
    y_ref = x64 / x64.norm(dim=1, keepdim=True)
    y_ref.backward(g.to(F64))
    u = 2.0 ** -24
    n_ref = x64.detach().norm(dim=1)
    yh, g64 = y_ref.detach(), g.to(F64)
    terms = (g64.abs() + yh.abs() * (yh.abs() * g64.abs()).sum(1, keepdim=True)) / n_ref[:, None]
    out = []
    if not bool(((norm.to(F64) - n_ref).abs() <= (D + 2) * u * n_ref)[rows].all()):
        out.append("norm")
    if not bool(((y.to(F64) - yh).abs() <= (D + 4) * u * yh.abs())[rows].all()):
        out.append("y")
    if not bool(((dx.to(F64) - x64.grad).abs() <= 4 * (D + 6) * u * terms)[rows].all()):          # (y enters twice, each with its own (D + 4) u; the dot product; the division)
        out.append("dx")
    return out, yh


@pytest.mark.parametrize("shape", [(4, 2048), (1, 8), (3, 1), (3, 63), (3, 64), (3, 65), (3, 2049)],
                         ids=["4x2048", "1x8", "3x1", "3x63", "3x64", "3x65", "3x2049"])
def test_l2norm_against_float64(pkg, shape):
    """mh_l2norm_fwd / mh_l2norm_bwd: y = x / ||x||, dx = (g - y (y . g)) / ||x||.  Bars from the f32 sums of D terms: the norm (and the dot
    product) within D 2^-24 relative (of sum|terms|), so an element within (D + 4) 2^-24 of its own size plus the dot product's share.
    D = 1, 63, 64, 65, 2049: a wave's 64-lane stride loop with idle lanes, exactly one trip, and one element into the next trip."""
    B, D = shape
    gen = torch.Generator().manual_seed(17 + D)
    x, g = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    y, norm, dx = _l2norm_launch(pkg, x, g)
    misses, _ = _l2norm_misses(x, g, y, norm, dx, torch.arange(B))
    assert not misses, misses


def test_l2norm_of_a_zero_row_is_nan_in_that_row_only(pkg):
    """No eps, as in the reference: a zero row is 0 / 0 = NaN, exactly what x / x.norm() gives in float64, its norm exactly 0; the rows
    around it stay inside their bars (a NaN does not cross rows)."""
    B, D = 3, 65
    gen = torch.Generator().manual_seed(23)
    x, g = torch.randn((B, D), generator=gen), torch.randn((B, D), generator=gen)
    x[1] = 0.0
    y, norm, dx = _l2norm_launch(pkg, x, g)
    misses, y_ref = _l2norm_misses(x, g, y, norm, dx, torch.tensor([0, 2]))
    assert not misses, misses
    assert bool(torch.isnan(y_ref[1]).all()) and bool(torch.isnan(y[1]).all())
    assert float(norm[1]) == 0.0 and bool(torch.isfinite(y[[0, 2]]).all()) and bool(torch.isfinite(dx[[0, 2]]).all())


# ---------------------------------------------------------------------------------------------------------------------
# B. the tower
# ---------------------------------------------------------------------------------------------------------------------

BARS = {"fp16": (1e-2, 5e-2), "bf16": (6e-2, 1.5e-1)}          # (ftol, gtol) of tests/test_resnet_gpu.py's tower test
LAYERS, SIZE, NUM_CLASSES, GROUPS = (1, 1, 1, 1), 64, 10, 32


class _RoundSTE(torch.autograd.Function):
    """x -> x rounded to the 16-bit storage type (straight-through); `gscale` > 0: an ACTIVATION, whose gradient the tower stores in 16 bits as
    well (scaled by `gscale`); 0: a weight, whose gradient is produced in f32.  (tests/test_basic_resnet_gpu.py's, restated.)"""

    @staticmethod
    def forward(ctx, x, dtype, gscale):
        ctx.dtype, ctx.gscale = dtype, gscale
        return x.to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        if ctx.gscale:
            g = (g * ctx.gscale).to(ctx.dtype).to(g.dtype) / ctx.gscale
        return g, None, None


def _ref_features(p, st, image, layers, training, storage, groups=GROUPS):
    """bottleneck ResNet with a grouped conv2 over a torchvision-keyed dict, in the arithmetic of its operands; `storage`: the tower's 16-bit
    storage points, straight-through -- weights, convolution inputs and outputs, BatchNorm (+ residual) (+ ReLU) outputs, and the gradients
    of those activations.  `st`: running statistics, updated in place when training."""
    gs = 8192.0 if storage == F16 else 1.0
    q = (lambda t: _RoundSTE.apply(t, storage, gs)) if storage is not None else (lambda t: t)
    qw = (lambda t: _RoundSTE.apply(t, storage, 0.0)) if storage is not None else (lambda t: t)

    def conv(x, w, **kw):
        return q(F.conv2d(q(x), qw(w), **kw))

    def bn(x, pfx):
        return F.batch_norm(x, st[pfx + ".running_mean"], st[pfx + ".running_var"], p[pfx + ".weight"], p[pfx + ".bias"], training, 0.1, 1e-5)

    x = q(F.relu(bn(conv(image, p["conv1.weight"], stride=2, padding=3), "bn1")))
    x = F.max_pool2d(x, 3, 2, 1)
    for li, (n, stride) in enumerate(zip(layers, (1, 2, 2, 2)), 1):
        for bi in range(n):
            L = f"layer{li}.{bi}."
            s = stride if bi == 0 else 1
            o = q(F.relu(bn(conv(x, p[L + "conv1.weight"]), L + "bn1")))
            o = q(F.relu(bn(conv(o, p[L + "conv2.weight"], stride=s, padding=1, groups=groups), L + "bn2")))
            o = bn(conv(o, p[L + "conv3.weight"]), L + "bn3")
            idn = x
            if (L + "downsample.0.weight") in p:
                idn = q(bn(conv(x, p[L + "downsample.0.weight"], stride=s), L + "downsample.1"))
            x = q(F.relu(o + idn))
    return x.mean(dim=(2, 3))


def _split_state(sd):
    p = {k: v.detach().cpu().to(F64) for k, v in sd.items() if "running_" not in k and "num_batches" not in k}
    st = {k: v.detach().cpu().to(F64).clone() for k, v in sd.items() if "running_" in k}
    return p, st


# The seed rule of tests/test_basic_resnet_gpu.py: picked on the CPU from the reference alone -- the smallest seed >= 11 for which the
# storage-rounded reference evaluated in float32 stays within 1.25 x deviation + 0.01 for every tensor and both dtypes; the test asserts
# it at the bar (1.5 x) before the GPU is touched.  SEEDS_REJECTED lists the seeds below SEED that did not qualify.
SEED = 11
SEEDS_REJECTED = ()


def _gradient_misses(grads, ref_grads, q_grads, factor=1.5):
    out = []
    for name, ref in ref_grads.items():
        den = float(ref.norm()) + 1e-12
        rel, sens = float((grads[name].to(F64) - ref).norm()) / den, float((q_grads[name] - ref).norm()) / den
        if rel > factor * sens + 0.01:
            out.append((name, round(rel, 4), round(sens, 4)))
    return out


@lru_cache(maxsize=None)
def _tower_reference(pkg, dtype, seed=SEED):
    T16 = F16 if dtype == "fp16" else BF16
    net = pkg.ResNeXt50_32x4d(num_classes=NUM_CLASSES, compute_dtype=dtype, layers=LAYERS, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for n, prm in net.named_parameters():          # BatchNorm affine parameters off their 1 / 0 defaults
        if prm.dim() == 1 and not n.startswith("fc."):
            prm.data = (torch.rand(prm.shape, generator=g) + 0.5) if n.endswith("weight") else torch.randn(prm.shape, generator=g) * 0.2
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    image = torch.randn((2, 3, SIZE, SIZE), generator=g)
    labels = torch.tensor([3, 8])
    p, st0 = _split_state(sd)

    def run(storage, arith=F64):
        leaves = {k: v.detach().to(arith).clone().requires_grad_(True) for k, v in p.items()}
        st = {k: v.to(arith).clone() for k, v in st0.items()}
        feats = _ref_features(leaves, st, image.to(arith), LAYERS, True, storage)
        logits = F.linear(feats, leaves["fc.weight"], leaves["fc.bias"])
        F.cross_entropy(logits, labels).backward()
        return logits.detach(), {k: v.grad for k, v in leaves.items()}, st
    return dict(sd=sd, image=image, labels=labels, plain=run(None), rounded=run(T16), rounded_f32=run(T16, F32), T16=T16)


def seed_qualifies(pkg, seed, factor=1.25):
    """the seed rule, on the CPU: no tensor of either dtype outside factor x deviation + 0.01 in the float32 evaluation"""
    for dtype in ("fp16", "bf16"):
        r = _tower_reference(pkg, dtype, seed)
        if _gradient_misses(r["rounded_f32"][1], r["plain"][1], r["rounded"][1], factor):
            return False
    return True


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_resnext_forward_backward_matches_float64(pkg, dtype):
    ftol, gtol = BARS[dtype]
    r = _tower_reference(pkg, dtype)
    ref_logits, ref_grads, _ = r["plain"]
    q_logits, q_grads, q_st = r["rounded"]
    assert not _gradient_misses(r["rounded_f32"][1], ref_grads, q_grads), "the reference misses its own bar in float32: SEED is no usable input"
    net = pkg.ResNeXt50_32x4d(num_classes=NUM_CLASSES, compute_dtype=dtype, layers=LAYERS)
    net.load_state_dict(r["sd"])
    net.cuda().train()
    assert {u.conv.cout // u.conv.groups for u in net._units if u.conv.grouped} == {4, 8, 16, 32}
    logits = net(r["image"].cuda())
    pkg.CrossEntropyLoss()(logits, r["labels"].cuda()).backward()
    torch.cuda.synchronize()
    got_logits = logits.detach().cpu().to(F64)
    err, errq = float((got_logits - ref_logits).abs().max()), float((got_logits - q_logits).abs().max())
    sens_f = float((q_logits - ref_logits).abs().max())
    tag = f"[resnext50_32x4d 1111@64 {dtype}]"
    parity_log(f"{tag} max |logit - float64| = {err:.3e} (vs the storage-rounded reference {errq:.3e}; storage rounding alone {sens_f:.3e}; "
               f"|logit| max {float(ref_logits.abs().max()):.3f})")
    assert err < ftol * max(1.0, float(ref_logits.abs().max())) and errq < 0.5 * ftol
    worst, worst_n, fails = ("", 0.0, 0.0), ("", 0.0), []
    for name, prm in net.named_parameters():
        got = prm.grad.detach().cpu().to(F64)
        den = float(ref_grads[name].norm()) + 1e-12
        rel = float((got - ref_grads[name]).norm()) / den
        sens = float((q_grads[name] - ref_grads[name]).norm()) / den
        nq = float(q_grads[name].norm())
        dn = abs(float(got.norm()) - nq) / (nq + 1e-30)
        if rel > worst[1]:
            worst = (name, rel, sens)
        if dn > worst_n[1]:
            worst_n = (name, dn)
        if rel > 1.5 * sens + 0.01:
            fails.append(f"{name}: |hip - float64| / |float64| = {rel:.3f}, storage rounding alone gives {sens:.3f}")
        if abs(float(got.norm()) - nq) > gtol * nq + 1e-7:
            fails.append(f"{name}: gradient norm off the storage-rounded reference's by {dn:.3f} (bar {gtol})")
    parity_log(f"{tag} worst gradient deviation from float64 {worst[1]:.3f} ({worst[0]}; 16-bit storage alone: {worst[2]:.3f}); "
               f"worst norm deviation from the storage-rounded reference {worst_n[1]:.3f} ({worst_n[0]})")
    assert not fails, fails[:6]
    sd = net.state_dict()
    for k, v in q_st.items():          # running statistics advance as nn.BatchNorm2d's (F.batch_norm's) do
        bar = (2e-3 if k.endswith("running_mean") else 2e-2) * max(1.0, float(v.abs().max()))
        assert float((sd[k].cpu().to(F64) - v).abs().max()) < bar, k
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked")) and int(sd["layer4.0.bn2.num_batches_tracked"]) == 1
    net.eval()          # eval mode: the running statistics; features against the float64 composition with the same statistics
    with torch.no_grad():
        feats = net.features(r["image"].cuda()).cpu().to(F64)
    p, st = _split_state(sd)
    ref_e = _ref_features(p, st, r["image"].to(F64), LAYERS, False, None)
    q_e = _ref_features(p, st, r["image"].to(F64), LAYERS, False, r["T16"])
    e, eq = float((feats - ref_e).abs().max()), float((feats - q_e).abs().max())
    parity_log(f"{tag} eval features: max |f - float64| = {e:.3e} (vs storage-rounded {eq:.3e}; |f| max {float(ref_e.abs().max()):.3f})")
    assert feats.shape == (2, 2048) and e < ftol * max(1.0, float(ref_e.abs().max())) and eq < 0.5 * ftol
    assert all(int(v) == 1 for k, v in net.state_dict().items() if k.endswith("num_batches_tracked"))


def test_resnext_gradients_accumulate_in_place_like_autograd(pkg):
    torch.manual_seed(1)
    net = pkg.ResNeXt50_32x4d(num_classes=10, compute_dtype="fp16", layers=LAYERS).cuda().train()
    g = torch.Generator().manual_seed(2)
    image = torch.randn((4, 3, 64, 64), generator=g).cuda()
    labels = torch.tensor([1, 7, 3, 3]).cuda()
    ce = pkg.CrossEntropyLoss()
    ce(net(image), labels).backward()
    first = {n: p.grad.clone() for n, p in net.named_parameters()}
    ce(net(image), labels).backward()          # .grad exists now: the in-place path (mh_gconv_wgrad with accumulate = 1 for the grouped layers)
    torch.cuda.synchronize()
    for n, p in net.named_parameters():
        ref = 2.0 * first[n]
        assert float((p.grad - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-12, n
    assert int(net.bn1.num_batches_tracked) == 2 and int(net.layer4[0].bn2.num_batches_tracked) == 2


def test_resnext_classifier_step_moves_every_parameter(pkg):
    torch.manual_seed(0)
    model = pkg.ResNetClassifier(num_labels=2, compute_dtype="fp16", arch="resnext50_32x4d", layers=LAYERS).cuda()
    assert type(model.resnet) is pkg.ResNeXt50_32x4d
    pkg.flatten_parameters(model)
    model.train()
    g = torch.Generator().manual_seed(3)
    batch = {"pixel_values": torch.randn((8, 3, 64, 64), generator=g).cuda(), "labels": torch.tensor([0, 1, 1, 0, 1, 0, 0, 1]).cuda()}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = pkg.Adam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    loss, logits = model(**batch)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert logits.shape == (8, 2) and np.isfinite(float(loss.detach()))
    for n, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[n]), n


def test_kevin_model_over_resnext(pkg):
    tc = pkg.TextConfig(vocab_size=600, hidden=128, layers=1, heads=2, intermediate=256, max_position=64)
    cc = pkg.TextConfig(vocab_size=500, hidden=128, layers=1, heads=2, intermediate=256, max_position=64)
    model = pkg.KevinMultimodalClassifier("concatenation", text=tc, image="resnext50_32x4d", caption=cc, proj=128, compute_dtype="fp16", seed=1,
                                          resnet_layers=LAYERS).cuda().train()
    assert type(model.image_model) is pkg.ResNeXt50_32x4d and model.image_fine_tune[0].in_features == 2048
    n, S = 4, 16
    g = torch.Generator().manual_seed(5)
    text, cap = torch.randint(5, 600, (n, S), generator=g), torch.randint(5, 500, (n, S), generator=g)
    mask = (torch.arange(S)[None] < torch.randint(4, S + 1, (n,), generator=g)[:, None]).long()
    image = torch.randn((n, 3, 64, 64), generator=g)
    out = model(*[t.cuda() for t in (text * mask, image, mask, cap * mask, mask)])
    pkg.SigmoidFocalLoss()(out, torch.tensor([0.0, 1.0, 1.0, 0.0]).cuda()).backward()
    torch.cuda.synchronize()
    assert out.shape == (n,) and bool(torch.isfinite(out).all())
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    groups = model.get_params(1e-3)
    image_ids = {id(p) for p in groups[2]["params"]}
    assert all(id(p) in image_ids for p in model.image_model.parameters()) and all(id(p) in image_ids for p in model.image_fine_tune.parameters())
    assert groups[2]["lr"] == pytest.approx(0.8e-3)


class _TorchBH(nn.Module):
    """ResNeXt50_32x4d_BH's head written with torch.nn (example_scripts/Untitled-2.py:164-179,226-237), over given features"""

    def __init__(self, D):
        super().__init__()
        self.fea_bn = nn.BatchNorm1d(D)
        self.fea_bn.bias.requires_grad_(False)
        self.fc = nn.Sequential(nn.Linear(D, 2))
        self.s = 1

    def forward(self, fea):
        fea = self.fea_bn(fea)
        fea = torch.div(fea, torch.norm(fea, 2, 1, True))
        return self.fc(fea) * self.s


def test_resnext_binary_head_model_against_torch_float64(pkg):
    """The head (fea_bn -> l2_norm -> Linear -> x s) in f32 on the device against torch.nn in float64 over the tower's own features.  Every op is
    a sum of at most D = 2048 f32 terms (error <= D 2^-24 of sum|terms|); six such ops are chained (three forward, three backward) and at
    B = 4 the BatchNorm's 1 / sigma amplifies a feature's error by up to ~sqrt(B): bar 6 * 2 * D 2^-24 = 3e-3 of a tensor's largest entry."""
    model = pkg.ResNeXt50_32x4d_BH(compute_dtype="fp16", layers=LAYERS, seed=3).cuda().train()
    g = torch.Generator().manual_seed(8)
    x = torch.randn((4, 3, 64, 64), generator=g).cuda()
    labels = torch.tensor([0, 1, 1, 0])
    with torch.no_grad():
        model.eval()
        feats = model.net.features(x)            # eval: the same features for both evaluations below
    D = feats.shape[1]
    ref = _TorchBH(D).double().train()
    ref.load_state_dict({"fea_bn." + k: v.cpu().double() for k, v in model.fea_bn.state_dict().items()}
                        | {"fc.0." + k: v.cpu().double() for k, v in model.binary_head.fc[0].state_dict().items()})
    f64 = feats.cpu().double().requires_grad_(True)
    ref_logits = ref(f64)
    F.cross_entropy(ref_logits, labels).backward()
    model.fea_bn.train(), model.binary_head.train()
    fd = feats.clone().requires_grad_(True)
    logits = model.binary_head(model.fea_bn(fd))
    pkg.CrossEntropyLoss()(logits, labels.cuda()).backward()
    torch.cuda.synchronize()
    bar = 12 * D * 2.0 ** -24

    def close(what, got, want):
        err, size = float((got.detach().cpu().double() - want).abs().max()), float(want.abs().max())
        parity_log(f"[resnext50_32x4d_BH] {what}: max error {err:.3e} of max |ref| {size:.3e} (bar {bar:.1e} of it)")
        assert err <= bar * size, what
    assert logits.shape == (4, 2)
    close("logits", logits, ref_logits.detach())
    close("d features", fd.grad, f64.grad)
    close("fea_bn.weight.grad", model.fea_bn.weight.grad, ref.fea_bn.weight.grad)
    close("binary_head.fc.0.weight.grad", model.binary_head.fc[0].weight.grad, ref.fc[0].weight.grad)
    close("binary_head.fc.0.bias.grad", model.binary_head.fc[0].bias.grad, ref.fc[0].bias.grad)
    close("fea_bn.running_mean", model.fea_bn.running_mean, ref.fea_bn.running_mean)
    assert model.fea_bn.bias.grad is None and ref.fea_bn.bias.grad is None
    # ... and the whole model: tower + head, one forward / backward
    model.train()
    model.zero_grad()
    out = model(x)
    pkg.CrossEntropyLoss()(out, labels.cuda()).backward()
    torch.cuda.synchronize()
    assert out.shape == (4, 2) and bool(torch.isfinite(out).all()) and model.fea_bn.bias.grad is None
    for name, p in model.named_parameters():
        if name not in ("fea_bn.bias", "fc.weight", "fc.bias"):          # (the frozen bias; the reference's unused `fc`)
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
