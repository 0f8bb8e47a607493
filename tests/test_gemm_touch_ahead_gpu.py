"""The product GEMM's K loop (csrc/gemm_tile.h: k_loop; csrc/gemm.hip: gemm_kernel), exact at the pipeline's edges.  Written for the
touch-ahead experiment (profiles/r25_gemm_touch_ahead.txt): a K loop that kept one vector load per wave in flight across its barrier, d K
tiles ahead of the LDS-DMA, and retired the DMA of the next K tile with a counted wait.  The touch was measured slower and is not in the
tree; what that work kept is that the K-strided fragment reads no longer wait for the DMA issued at the top of their K step, so the two
LDS stages really overlap in the dgrad and wgrad layouts.  What can go wrong in such a loop is a stage read before it landed, a stage
overwritten while it is still read, or a prologue / drain that miscounts when there are fewer K tiles than the pipeline is deep; D = 3
below is the touch distance the trip counts were chosen around.  Operands are integers in [-4, 4]: every product is at most 16 and every
sum of at most 768 of them stays below 2^24, so the f32 accumulators are exact and the result must equal the float64 product (rounded
once to the 16-bit output type where the output is 16-bit) bit for bit.  Every output has 64 sentinel elements in front of it and behind
it, which must not change.
(M <= 64 would go to gemm_skinny_kernel in the forward and dgrad layouts; those problems carry a device-side row count equal to M,
which keeps them on gemm_kernel.  The weight-gradient layout needs M % 8 == 0: its row counts are 8, 120 and 136.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
BOTH = pytest.mark.parametrize("T16", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
LAYOUTS = pytest.mark.parametrize("layout", ["fwd", "dgrad", "wgrad"])
BK, GUARD = 64, 64
SENT16, SENT32 = 7.0, 7.0


D = 3
NKS = sorted({1, 2, D - 1, D, D + 1, D + 2, 12} - {0})
KMAX, RMAX = 12 * BK, 256


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_propaganda_meme_classification_amd import ops as _ops
    return _ops


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bank():
    """The integer operands every case slices, made once (float64, host): row-major [rows][k] and k-major [k][rows] for both sides."""
    g = torch.Generator(device="cpu").manual_seed(1234)
    mk = lambda *s, lo=-4, hi=5: torch.randint(lo, hi, s, generator=g).to(F64)
    return {"a_rk": mk(RMAX, KMAX), "b_rk": mk(RMAX, KMAX), "a_kr": mk(KMAX, RMAX), "b_kr": mk(KMAX, RMAX),
            "bias": mk(RMAX, lo=-3, hi=4), "res": mk(RMAX, RMAX, lo=-8, hi=9), "pos_a": mk(RMAX, KMAX, lo=0, hi=2), "pos_b": mk(RMAX, KMAX, lo=0, hi=2)}


class Guarded:
    """an output tensor with GUARD sentinel elements in front of it and behind it"""

    def __init__(self, shape, dtype, fill):
        n = 1
        for s in shape:
            n *= s
        self.fill = fill
        self.flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev())
        self.t = self.flat[GUARD:GUARD + n].view(*shape)

    def bands_intact(self):
        return bool((self.flat[:GUARD] == self.fill).all()) and bool((self.flat[-GUARD:] == self.fill).all())


def _problem(ops, bank, layout, M, N, K, T16, a_key=None, b_key=None, **kw):
    """(Gemm, outputs, float64 product [M, N], float64 row sums of A) of one problem in `layout`; K is the contraction length"""
    if layout == "wgrad":
        a64, b64 = bank[a_key or "a_kr"][:K, :M].contiguous(), bank[b_key or "b_kr"][:K, :N].contiguous()
        ref, lda, ldb = a64.t() @ b64, M, N
        rs = a64.sum(0)
    elif layout == "dgrad":
        a64, b64 = bank[a_key or "a_rk"][:M, :K].contiguous(), bank[b_key or "b_kr"][:K, :N].contiguous()
        ref, lda, ldb = a64 @ b64, K, N
        rs = None
    else:
        a64, b64 = bank[a_key or "a_rk"][:M, :K].contiguous(), bank[b_key or "b_rk"][:N, :K].contiguous()
        ref, lda, ldb = a64 @ b64.t(), K, K
        rs = None
    A, B = a64.to(T16).to(dev()), b64.to(T16).to(dev())
    outs = {}
    if layout == "wgrad" or kw.get("ksplit", 0) > 1:
        sp = max(kw.get("ksplit", 0), 1)
        outs["C"] = Guarded((sp, M, N) if sp > 1 else (M, N), F32, SENT32)
        if layout == "wgrad" and sp == 1:
            outs["rowsum"] = Guarded((M,), F32, SENT32)
            kw["rowsum"] = outs["rowsum"].t
    else:
        outs["C"] = Guarded((M, N), T16, SENT16)
    if layout != "wgrad" and M <= 64 and "rows_dev" not in kw and kw.get("ksplit", 0) <= 1:
        kw["rows_dev"] = torch.tensor([M], dtype=torch.int32, device=dev())      # not eligible for gemm_skinny_kernel
    return ops.Gemm(A, B, outs["C"].t, M, N, K, lda, ldb, N, **kw), outs, ref, rs


def _launch(ops, layout, problems):
    ops.gemm_grouped(problems, layout == "wgrad", layout != "fwd")


def _check(outs, ref, rs, T16, what):
    C = outs["C"].t
    want = ref.to(C.dtype).to(dev())      # integers below 2^24: exact in f32, rounded once to a 16-bit output as the kernel rounds its f32 sum
    assert torch.equal(C, want), what
    if "rowsum" in outs:
        assert torch.equal(outs["rowsum"].t, rs.to(F32).to(dev())), what + ": row sums"
    for k, o in outs.items():
        assert o.bands_intact(), f"{what}: guard band of {k} changed"


@BOTH
@LAYOUTS
@pytest.mark.parametrize("nk", NKS)
def test_every_trip_count_around_the_touch_distance(ops, bank, layout, nk, T16):
    """nk K tiles, nk in {1, 2, d-1, d, d+1, d+2, 12}: fewer tiles than d is where the prologue and the drain can go wrong; ragged M over
    one and two row panels, a partial and a second column tile"""
    for M in ((8, 120, 136) if layout == "wgrad" else (1, 127, 129)):
        for N in (8, 136):
            p, outs, ref, rs = _problem(ops, bank, layout, M, N, nk * BK, T16)
            _launch(ops, layout, [p])
            _check(outs, ref, rs, T16, f"{layout} M={M} N={N} nk={nk}")


@BOTH
def test_wgrad_ragged_contraction_reads_zeros(ops, bank, T16):
    """a contraction of 100 rows: the second K tile holds 36 rows and 28 that read as zeros"""
    p, outs, ref, rs = _problem(ops, bank, "wgrad", 136, 136, 100, T16)
    _launch(ops, "wgrad", [p])
    _check(outs, ref, rs, T16, "wgrad K=100")


@BOTH
@LAYOUTS
def test_live_row_count_changes_between_launches(ops, bank, layout, T16):
    """a problem laid out for 256 rows; the live count changes ON THE DEVICE between launches of the same prepared call: 0 (no tile
    runs / an empty contraction: nk = 0), 1, 65 and all of them"""
    R, K = 256, (D + 2) * BK
    rows = torch.zeros(1, dtype=torch.int32, device=dev())
    if layout == "wgrad":      # the contraction runs over the packed rows
        p, outs, _, _ = _problem(ops, bank, layout, 136, 136, R, T16, rows_dev=rows)
        a64, b64 = bank["a_kr"][:R, :136], bank["b_kr"][:R, :136]
    else:
        p, outs, ref, _ = _problem(ops, bank, layout, R, 136, K, T16, rows_dev=rows)
    for live in (0, 1, 65, R):
        rows.fill_(live)
        for o in outs.values():
            o.flat.fill_(o.fill)
        _launch(ops, layout, [p])
        if layout == "wgrad":
            _check(outs, a64[:live].t() @ b64[:live], a64[:live].sum(0), T16, f"wgrad live={live}")
        else:
            C = outs["C"].t
            assert torch.equal(C[:live], ref[:live].to(T16).to(dev())), f"{layout} live={live}"
            assert bool((C[live:] == SENT16).all()), f"{layout} live={live}: rows past the live count are not stored"
            assert outs["C"].bands_intact()


@BOTH
@pytest.mark.parametrize("layout", ["fwd", "wgrad"])
@pytest.mark.parametrize("ksplit", [2, 3])
def test_split_k_slabs(ops, bank, layout, ksplit, T16):
    """K = 448 = 7 K tiles in 2 (4 + 3) and 3 (3 + 3 + 1) splits: every slab is the exact product over its own chunk"""
    from multimodal_propaganda_meme_classification_amd import _lib
    M, N, K = 136, 136, 448
    assert _lib.load("bf16").mh_gemm_ksplit_for(K, ksplit) == ksplit
    p, outs, _, _ = _problem(ops, bank, layout, M, N, K, T16, ksplit=ksplit)
    _launch(ops, layout, [p])
    chunk = ((K + ksplit - 1) // ksplit + BK - 1) // BK * BK
    for s in range(ksplit):
        k0, k1 = s * chunk, min(K, (s + 1) * chunk)
        if layout == "wgrad":
            want = bank["a_kr"][k0:k1, :M].t() @ bank["b_kr"][k0:k1, :N]
        else:
            want = bank["a_rk"][:M, k0:k1] @ bank["b_rk"][:N, k0:k1].t()
        assert torch.equal(outs["C"].t[s], want.to(F32).to(dev())), f"{layout} slab {s} of {ksplit}"
    assert outs["C"].bands_intact()


@BOTH
@LAYOUTS
def test_grouped_launch_with_different_trip_counts(ops, bank, layout, T16):
    """two problems in one launch, nk = 1 and nk = d + 2: the workgroups of one launch run different trip counts"""
    M, N = (136, 136) if layout == "wgrad" else (129, 136)
    p1, o1, r1, s1 = _problem(ops, bank, layout, M, N, BK, T16)
    p2, o2, r2, s2 = _problem(ops, bank, layout, M, N, (D + 2) * BK, T16)
    _launch(ops, layout, [p1, p2])
    _check(o1, r1, s1, T16, f"{layout} nk=1 beside nk={D + 2}")
    _check(o2, r2, s2, T16, f"{layout} nk={D + 2} beside nk=1")


@BOTH
def test_epilogues_behind_the_counted_waits(ops, bank, T16):
    """bias + residual, and the GELU epilogue with its aux copy: the epilogue's f32 staging tile re-uses the K stages, so it must not be
    written while a DMA could still land there.  GELU case: non-negative operands and a bias of 8 make every pre-activation v >= 8, where
    GELU(v) = v * Phi(v) differs from v by less than 1e-14 relative -- the float64 GELU rounded to 16 bits is v itself."""
    M, N, K = 129, 136, (D + 1) * BK
    bias64, res64 = bank["bias"][:N], bank["res"][:M, :N]
    bias, res = bias64.to(F32).to(dev()), res64.to(T16).to(dev())
    p, outs, ref, _ = _problem(ops, bank, "fwd", M, N, K, T16, bias=bias, residual=res)
    _launch(ops, "fwd", [p])
    _check(outs, ref + bias64 + res64, None, T16, "bias + residual")

    aux = Guarded((M, N), T16, SENT16)
    bias8 = torch.full((N,), 8.0, dtype=F32, device=dev())
    p, outs, ref, _ = _problem(ops, bank, "fwd", M, N, K, T16, a_key="pos_a", b_key="pos_b", bias=bias8, aux=aux.t, gelu=True)
    outs["aux"] = aux
    _launch(ops, "fwd", [p])
    v = ref + 8.0
    assert float(v.max()) <= 256, "every pre-activation is an integer both 16-bit types hold exactly"
    assert torch.equal(aux.t, v.to(T16).to(dev())), "aux = the pre-activation"
    _check(outs, torch.nn.functional.gelu(v), None, T16, "GELU epilogue")
