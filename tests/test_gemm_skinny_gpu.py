"""The skinny-M GEMM kernel (csrc/gemm.hip: gemm_skinny_kernel) behind mh_gemm_bf16_grouped: grouped launches whose problems all
have M <= 64 rows, layouts forward (0,0) and dgrad (0,1) -- the [B, D] panels of the compact last encoder layer and the caption
decoder's step.  One wave owns BN = 16 output columns and keeps D K tiles of 64 in flight in a register ring (D = 8 for M <= 32,
4 for M <= 64).  Checked here:
  * exact integer results over M x N x K around every edge of the tile, the ring and the 16-row block, with lda > K, ldc > N and
    outputs that are column slices of a wider buffer;
  * the SAME BITS as gemm_kernel on N(0, 1) operands for every epilogue the step and the decoder use: the reference is the same
    problem with 65+ rows (a GEMM output row depends on its own A row only), which mh_gemm_skinny_eligible proves took gemm_kernel;
  * grouped launches of unlike problems, the M = 64 / 65 boundary, nothing written outside the result, and the dispatch rule itself.
(reference call sites: every nn.Linear behind Multimodal_example_task2C.txt:175,183 and loss.backward() :216)"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = torch.float32
BOTH = pytest.mark.parametrize("T16", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
LAYOUTS = pytest.mark.parametrize("bk", [False, True], ids=["fwd", "dgrad"])
BN = 16                                   # column tile of the skinny kernel
DEPTHS = (8, 4)                           # K tiles in flight: M <= 32, M <= 64
MS = (1, 16, 17, 32, 33, 64)
NS = sorted({8, BN - 8, BN, BN + 8, 768})
KS = sorted({64, 3072} | {64 * (d + o) for d in DEPTHS for o in (-1, 0, 1)})


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from multimodal_propaganda_meme_classification_amd import ops as _ops
    return _ops


def dev():
    return torch.device("cuda:0")


def _lib(T16):
    from multimodal_propaganda_meme_classification_amd import _lib as L
    return L.load("bf16" if T16 == torch.bfloat16 else "fp16")


def eligible(T16, problems, bk, ak=False):
    """mh_gemm_skinny_eligible on the descriptors ops.gemm_grouped would build (host only: nothing is launched)"""
    from multimodal_propaganda_meme_classification_amd import _lib as L
    arr = (L.MhGemmProblem * len(problems))()
    for a, g in zip(arr, problems):
        a.A, a.B, a.C = g.A.data_ptr(), g.B.data_ptr(), g.C.data_ptr()
        a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.flags, a.alpha = g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.flags, g.alpha
        if g.drop is not None:
            a.drop_rng, a.drop_p, a.drop_stream = g.drop[0].data_ptr(), float(g.drop[1]), int(g.drop[2])
        if g.rows_dev is not None:
            a.rows_dev = g.rows_dev.data_ptr()
        a.ksplit = g.ksplit
    return int(_lib(T16).mh_gemm_skinny_eligible(arr, len(problems), int(ak), int(bk)))


def ints_cpu(*shape, lo=-1, hi=2, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g)


_INT_CACHE = {}


def int_case(M, N, K, bk):
    """integer operands (CPU, f32: every value below is an integer under 2^24, so f32 arithmetic is exact) and their product,
    computed once per shape and left unchanged"""
    key = (M, N, K, bk)
    if key not in _INT_CACHE:
        A = ints_cpu(M, K, seed=1 + M).float()
        B = (ints_cpu(K, N, seed=2 + N) if bk else ints_cpu(N, K, seed=2 + N)).float()
        _INT_CACHE[key] = (A, B, A @ B if bk else A @ B.t())
    return _INT_CACHE[key]


def wide(t, pad, T):
    """t as the leading columns of a buffer `pad` columns wider: (buffer, leading dimension)"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), 3.0, dtype=T, device=dev())
    buf[:, :t.shape[1]] = t.to(T)
    return buf, t.shape[1] + pad


@BOTH
@LAYOUTS
def test_exact_on_integers_over_every_edge(ops, T16, bk):
    """Operands in {-1, 0, 1}: every product and partial sum is an integer of magnitude <= K <= 3072 -- exact in f32.  The 16-bit
    output is checked as well wherever the CPU product stays within +-256 (integers up to 256 are exact in bf16 and fp16; the
    bound is evaluated on the CPU result, not assumed).  A has lda = K + 64; C is a column slice (offset 16, ldc = N + 40) of a
    wider buffer."""
    OFF, PAD = 16, 40
    for M in MS:
        for N in NS:
            for K in KS:
                A, B, ref = int_case(M, N, K, bk)
                Ab, lda = wide(A, 64, T16)
                Bd = B.to(T16).to(dev())
                ldb = N if bk else K
                want = ref.to(F32).to(dev())
                outs = [F32] + ([T16] if int(ref.abs().max()) <= 256 else [])
                assert K > 192 or len(outs) == 2
                for TO in outs:
                    buf = torch.full((M, N + PAD), 7.0, dtype=TO, device=dev())
                    p = ops.Gemm(Ab, Bd, buf.view(-1)[OFF:], M, N, K, lda, ldb, N + PAD)
                    assert eligible(T16, [p], bk) == 1
                    ops.gemm_grouped([p], False, bk)
                    tag = f"M={M} N={N} K={K} out={TO}"
                    assert torch.equal(buf[:, OFF:OFF + N].float(), want), tag
                    assert bool((buf[:, :OFF] == 7.0).all()) and bool((buf[:, OFF + N:] == 7.0).all()), "columns around the slice: " + tag


def _rand(shape, seed, T, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(T).to(dev())


EPILOGUES = {
    "none": dict(),
    "bias": dict(bias=1),
    "bias_alpha": dict(bias=1, alpha=0.37),
    "bias_residual": dict(bias=1, residual=1),
    "bias_residual_aux": dict(bias=1, residual=1, aux=1),
    "bias_gelu_deriv_aux": dict(bias=1, aux=1, gelu=True, deriv_aux=True),
    "bias_quick_gelu_deriv_aux": dict(bias=1, aux=1, gelu=True, deriv_aux=True, quick=True),
    "bias_gelu": dict(bias=1, gelu=True),
    "mul_deriv_aux": dict(mul=1, deriv_aux=True),
    "mul_residual": dict(mul=1, residual=1, deriv_aux=True),
    "mul_dgelu": dict(mul=1),
    "mul_dquick_gelu": dict(mul=1, quick=True),
    "f32": dict(f32=True, bias=1),
    "f32_accum": dict(f32=True, accum=True),
}


@BOTH
@LAYOUTS
@pytest.mark.parametrize("K", [64, 3072])
def test_same_bits_as_gemm_kernel_on_real_values(ops, T16, bk, K):
    """N(0, 1) operands: the order of the sums shows in the last bit.  Reference: the same rows as the head of an 80-row problem, which
    takes gemm_kernel (asserted through mh_gemm_skinny_eligible -- without that the comparison would prove nothing)."""
    N, MREF = 200, 80
    A = _rand((MREF, K), 11, T16)
    B = _rand((K, N) if bk else (N, K), 12, T16)
    ldb = N if bk else K
    bias = _rand((N,), 13, F32)
    res = _rand((MREF, N), 14, T16)
    mul = _rand((MREF, N), 15, T16)
    c0 = _rand((MREF, N), 16, F32)
    for M in (17, 64):
        for name, e in EPILOGUES.items():
            got = {}
            for rows in (M, MREF):
                TO = F32 if e.get("f32") else T16
                out = c0.clone() if e.get("accum") else torch.full((MREF, N), 7.0, dtype=TO, device=dev())
                aux = torch.full((MREF, N), 5.0, dtype=T16, device=dev()) if e.get("aux") else None
                p = ops.Gemm(A, B, out, rows, N, K, K, ldb, N, bias=bias if e.get("bias") else None, residual=res if e.get("residual") else None,
                             aux=aux, mul=mul if e.get("mul") else None, gelu=e.get("gelu", False), quick=e.get("quick", False),
                             deriv_aux=e.get("deriv_aux", False), accum=e.get("accum", False), alpha=e.get("alpha", 1.0))
                assert eligible(T16, [p], bk) == (1 if rows == M else 0), (name, rows)
                ops.gemm_grouped([p], False, bk)
                got[rows] = (out, aux)
            tag = f"{name} M={M} K={K}"
            assert torch.equal(got[M][0][:M], got[MREF][0][:M]), tag
            assert bool(torch.isfinite(got[M][0][:M].float()).all()), tag
            if got[M][1] is not None:
                assert torch.equal(got[M][1][:M], got[MREF][1][:M]), "aux: " + tag
                assert bool((got[M][1][M:] == 5.0).all()), "aux rows past M: " + tag
            if not e.get("accum"):
                assert bool((got[M][0][M:] == 7.0).all()), "rows past M: " + tag
            else:
                assert torch.equal(got[M][0][M:], c0[M:]), "rows past M: " + tag


@BOTH
@LAYOUTS
def test_grouped_launches_of_unlike_problems(ops, T16, bk):
    """Eight problems in one launch, each with its own M, N and K (f32 outputs: exact at every K); then the same list with one problem
    of 70 rows -- not eligible any more, and still exact."""
    shapes = [(3, 24, 64), (33, 768, 192), (1, 8, 3072), (64, 40, 576), (17, 16, 512), (32, 200, 256), (16, 8, 64), (48, 136, 448)]
    def problems(shapes):
        ps, wants = [], []
        for M, N, K in shapes:
            A, B, ref = int_case(M, N, K, bk)
            out = torch.full((M, N), 7.0, dtype=F32, device=dev())
            ps.append(ops.Gemm(A.to(T16).to(dev()), B.to(T16).to(dev()), out, M, N, K, K, N if bk else K, N))
            wants.append(ref.to(F32).to(dev()))
        return ps, wants
    for n in (2, 8):
        ps, wants = problems(shapes[:n])
        assert eligible(T16, ps, bk) == 1
        ops.gemm_grouped(ps, False, bk)
        for p, w in zip(ps, wants):
            assert torch.equal(p.C, w), (n, p.M, p.N, p.K)
    ps, wants = problems(shapes[:3] + [(70, 24, 128)])
    assert eligible(T16, ps, bk) == 0, "one problem with M > 64 sends the whole group to gemm_kernel"
    ops.gemm_grouped(ps, False, bk)
    for p, w in zip(ps, wants):
        assert torch.equal(p.C, w), (p.M, p.N, p.K)


@BOTH
@LAYOUTS
@pytest.mark.parametrize("M,N,K", [(1, 8, 64), (17, 24, 320), (33, 768, 64), (64, 8, 576)])
def test_nothing_outside_the_result_is_written(ops, T16, bk, M, N, K):
    """Output, aux and 4096 elements behind each are pre-filled with a sentinel: rows >= M, columns >= N and the guard keep it."""
    ROWS, LDC, GUARD, S = M + 9, N + 24, 4096, 9.0
    A, B, ref = int_case(M, N, K, bk)
    Ad = torch.zeros((ROWS, K), dtype=T16, device=dev())
    Ad[:M] = A.to(T16)
    Ad[M:] = 1.0                                     # rows past M hold data: they must not be computed into anything stored
    Bd = B.to(T16).to(dev())
    for TO in (F32, T16):
        cbuf = torch.full((ROWS * LDC + GUARD,), S, dtype=TO, device=dev())
        abuf = torch.full((ROWS * LDC + GUARD,), S, dtype=T16, device=dev())
        ops.gemm_grouped([ops.Gemm(Ad, Bd, cbuf, M, N, K, K, N if bk else K, LDC, aux=abuf)], False, bk)
        for name, buf in (("C", cbuf), ("aux", abuf)):
            body = buf[:ROWS * LDC].view(ROWS, LDC)
            if TO == F32 and name == "C":
                assert torch.equal(body[:M, :N], ref.to(F32).to(dev())), name
            assert bool((body[M:] == S).all()), f"{name}: rows >= M"
            assert bool((body[:, N:] == S).all()), f"{name}: columns >= N"
            assert bool((buf[ROWS * LDC:] == S).all()), f"{name}: guard"


@BOTH
@LAYOUTS
def test_the_boundary_m64_m65(ops, T16, bk):
    N, K = 136, 320
    A, B, ref = int_case(65, N, K, bk)
    Ad, Bd = A.to(T16).to(dev()), B.to(T16).to(dev())
    for M, want in ((64, 1), (65, 0)):
        out = torch.full((65, N), 7.0, dtype=F32, device=dev())
        p = ops.Gemm(Ad, Bd, out, M, N, K, K, N if bk else K, N)
        assert eligible(T16, [p], bk) == want
        ops.gemm_grouped([p], False, bk)
        assert torch.equal(out[:M], ref[:M].to(F32).to(dev())), M
        assert bool((out[M:] == 7.0).all()), M


@BOTH
def test_dispatch_rule_fall_backs(ops, T16):
    """Host only: rows_dev, split-K, a dropout generator, the weight-gradient layout, M > 64 and very wide groups keep gemm_kernel."""
    M, N, K = 32, 64, 128
    A = torch.zeros((M, K), dtype=T16, device=dev())
    B = torch.zeros((N, K), dtype=T16, device=dev())
    out = torch.zeros((4, M, N), dtype=F32, device=dev())
    rows = torch.tensor([M], dtype=torch.int32, device=dev())
    rng = torch.zeros(4, dtype=torch.int32, device=dev())
    sp = _lib(T16).mh_gemm_ksplit_for(K, 2)
    assert sp == 2
    assert eligible(T16, [ops.Gemm(A, B, out, M, N, K, K, K, N)], False) == 1
    assert eligible(T16, [ops.Gemm(A, B, out, M, N, K, K, N, N)], True) == 1
    assert eligible(T16, [ops.Gemm(A, B, out, M, N, K, K, K, N, rows_dev=rows)], False) == 0
    assert eligible(T16, [ops.Gemm(A, B, out, M, N, K, K, K, N, ksplit=sp)], False) == 0
    assert eligible(T16, [ops.Gemm(A, B, out, M, N, K, K, K, N, drop=(rng, 0.1, 3))], False) == 0
    assert eligible(T16, [ops.Gemm(A, B, out, M, N, K, K, K, N)], True, ak=True) == 0
    assert eligible(T16, [ops.Gemm(A, B, out, M, N, K, K, K, N), ops.Gemm(A, B, out, M, N, K, K, K, N, rows_dev=rows)], False) == 0
    assert eligible(T16, [ops.Gemm(A, B, out, 65, N, K, K, K, N)], False) == 0
    # the width bound: 128 or more 128-column tiles in the group fill the chip on gemm_kernel (the decoder's logits GEMM)
    wide = lambda n: ops.Gemm(A, B, out, M, n, K, K, K, n)
    assert eligible(T16, [wide(127 * 128)], False) == 1 and eligible(T16, [wide(127 * 128 + 8)], False) == 0
    assert eligible(T16, [wide(64 * 128), wide(63 * 128)], False) == 1 and eligible(T16, [wide(64 * 128), wide(64 * 128)], False) == 0
