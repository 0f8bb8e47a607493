"""Per-shape time of the skinny-M GEMM kernel against gemm_kernel on the same buffers, weights cold (the method of tools/gemm_shapes.py
and tools/gemm_cold_probe.py): the six [B, D] panel launches of the compact last encoder layer at config 3 (two towers per launch,
M = 32, the step's epilogues) and the caption decoder's six forward shapes (M = 64).  The same problems with M = 65 rows take
gemm_kernel -- one row panel, the same weight traffic -- which mh_gemm_skinny_eligible confirms for every pair.

    python tools/gemm_skinny_shapes.py [--dtype fp16] [--rounds 5] [--config 3|5]

One measurement = HIP events around 7 launches, each on its own copy of the weights, after a 1-GiB fill has evicted them and the
activation panel has been read back in (in the step the panel was just written and the weights were last read a pass ago); median over
the rounds.  To compare another build of the library (other column tile / ring depth), load it through MEMEHIP_LIB_F16 / MEMEHIP_LIB.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from multimodal_propaganda_meme_classification_amd import ops, _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="fp16")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--tag", default="")
ap.add_argument("--sweep", action="store_true", help="instead of the twelve shapes: N = 4096 .. 24576 at K = D, M = 64 (the width bound of the dispatch rule)")
args = ap.parse_args()

dev = torch.device("cuda")
T16 = torch.float16 if args.dtype == "fp16" else torch.bfloat16
lib = _lib.load(args.dtype)
D, I = (1024, 4096) if args.config == 5 else (768, 3072)
COPIES, MREF = 7, 65
flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)      # 1 GiB


def rnd(*s, scale=0.5):
    return (torch.randn(*s, device=dev) * scale).to(T16)


def case(N, K, bk, towers, **epi):
    """COPIES launches' worth of problems (rows = MREF allocated): [copy][tower] -> kwargs of ops.Gemm without M"""
    xs = [rnd(MREF, K) for _ in range(towers)]
    out = []
    for _ in range(COPIES):
        ps = []
        for x in xs:
            w = rnd(K, N, scale=0.05) if bk else rnd(N, K, scale=0.05)
            kw = {}
            if epi.get("bias"):
                kw["bias"] = torch.randn(N, device=dev)
            if epi.get("residual"):
                kw["residual"] = rnd(MREF, N)
            if epi.get("gelu"):
                kw.update(aux=torch.empty((MREF, N), dtype=T16, device=dev), gelu=True, deriv_aux=True)
            if epi.get("mul"):
                kw.update(mul=rnd(MREF, N), deriv_aux=True)
            ps.append((x, w, torch.empty((MREF, N), dtype=T16, device=dev), N, K, K, N if bk else K, N, kw))
        out.append(ps)
    return out, bk, xs


def problems(ps, M):
    return [ops.Gemm(x, w, y, M, N, K, lda, ldb, ldc, **kw) for (x, w, y, N, K, lda, ldb, ldc, kw) in ps]


def eligible(ps, bk):
    arr = (_lib.MhGemmProblem * len(ps))()
    for a, g in zip(arr, ps):
        a.A, a.B, a.C, a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.flags = g.A.data_ptr(), g.B.data_ptr(), g.C.data_ptr(), g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.flags
    return int(lib.mh_gemm_skinny_eligible(arr, len(ps), 0, int(bk)))


V = 30528      # the caption decoder's padded vocabulary
cases = {
    # the compact last layer (engine.py: [B, D] panels of both towers, B = 32)
    f"last fwd out-proj  N{D} K{D}": (32, case(D, D, False, 2, bias=True, residual=True)),
    f"last fwd ffn-up    N{I} K{D}": (32, case(I, D, False, 2, bias=True, gelu=True)),
    f"last fwd ffn-down  N{D} K{I}": (32, case(D, I, False, 2, bias=True, residual=True)),
    f"last dgrad ffn-down N{I} K{D}": (32, case(I, D, True, 2, mul=True)),
    f"last dgrad ffn-up  N{D} K{I}": (32, case(D, I, True, 2, residual=True)),
    f"last dgrad out-proj N{D} K{D}": (32, case(D, D, True, 2)),
    # the caption decoder's step (blip.py), 64 sequences
    f"decode qkv         N{3 * D} K{D}": (64, case(3 * D, D, False, 1, bias=True)),
    f"decode proj        N{D} K{D}": (64, case(D, D, False, 1, bias=True)),
    f"decode proj + res  N{D} K{D}": (64, case(D, D, False, 1, bias=True, residual=True)),
    f"decode ffn-up      N{I} K{D}": (64, case(I, D, False, 1, bias=True, gelu=True)),
    f"decode ffn-down    N{D} K{I}": (64, case(D, I, False, 1, bias=True, residual=True)),
    f"decode logits      N{V} K{D}": (64, case(V, D, False, 1, bias=True)),
}
if args.sweep:      # where the dispatch rule's width bound sits: one problem, M = 64, N from the FFN's width to the vocabulary's
    cases = {f"sweep fwd          N{n} K{D}": (64, case(n, D, False, 1, bias=True)) for n in (4096, 6144, 8192, 12288, 16384, 24576)}


def measure(launches, bk, xs):
    flush.fill_(1.0)
    for x in xs:
        x.float().sum()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for ps in launches:
        ops.gemm_grouped(ps, False, bk)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / len(launches)


print(f"# tools/gemm_skinny_shapes.py {args.tag} --dtype {args.dtype} --config {args.config}: us per launch, median of {args.rounds} x {COPIES} launches, "
      f"weights cold; {torch.cuda.get_device_name(0)}")
tot = {"skinny": 0.0, "gemm_kernel": 0.0}
for name, (M, (copies, bk, xs)) in cases.items():
    small = [problems(ps, M) for ps in copies]
    big = [problems(ps, MREF) for ps in copies]
    took = "skinny" if eligible(small[0], bk) else "gemm_kernel"      # (the rule sends very wide launches to gemm_kernel at any M)
    assert eligible(big[0], bk) == 0
    for l in (small[0], big[0]):
        ops.gemm_grouped(l, False, bk)
    ts, tb = [], []
    for _ in range(args.rounds):
        ts.append(measure(small, bk, xs))
        tb.append(measure(big, bk, xs))
    ts.sort(), tb.sort()
    ms, mb = ts[len(ts) // 2], tb[len(tb) // 2]
    if name.startswith("last"):
        assert took == "skinny"
        tot["skinny"] += ms
        tot["gemm_kernel"] += mb
    print(f"{name:34s} M={M:2d} {took} {ms:7.1f} us [{ts[0]:6.1f}..{ts[-1]:6.1f}] | M={MREF} gemm_kernel {mb:7.1f} us [{tb[0]:6.1f}..{tb[-1]:6.1f}] | x{mb / ms:5.2f}", flush=True)
print("sum of the six compact-layer launches (us):", {k: round(v, 1) for k, v in tot.items()})
