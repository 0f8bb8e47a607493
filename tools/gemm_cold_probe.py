"""What cache state costs the grouped GEMM launches of config 3.  All ten launch shapes of a layer pair (text + image tower in one launch): the
four forward ones, their four dgrad ones and the two weight-gradient launches, each timed in four cache states: everything hot (back-to-back
repeats, what tools/gemm_shapes.py times), everything evicted (a 1-GiB fill before the launch), only operand B cold (evict, then read A),
only operand A cold.  B is the weight in the forward and dgrad layouts; in the step the activations were just written by the previous
kernel and the weights were last read a whole pass ago (342 MB of 16-bit weights per pass against a 256-MB Infinity Cache).  The
weight-gradient launches read two activations, the older of them written a whole pass ago.  One launch per measurement, HIP events,
median of 9.
    python tools/gemm_cold_probe.py [NAME=libmemehip_f16.so ...] [--out FILE]
Several builds of the fp16 library are timed in ONE process, alternating per shape and cache state (the order flips every repeat); with
no argument the package's own build is timed."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from multimodal_propaganda_meme_classification_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda")
T16 = torch.float16
Tt, Ti, D, I = 2096, 6304, 768, 3072
REPS = 9
flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)      # 1 GiB


def load_build(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (restype, argtypes) in _lib._SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def rnd(*s, scale=0.5):
    return (torch.randn(*s, device=dev) * scale).to(T16)


def case(N, K, bk):
    """forward (bk False: weights [N][K]) or dgrad (bk True: weights [K][N]) of one linear layer, both towers"""
    ps, a_ops, b_ops = [], [], []
    for T in (Tt, Ti):
        x = rnd(T, K)
        w = rnd(K, N, scale=0.05) if bk else rnd(N, K, scale=0.05)
        y = torch.empty((T, N), dtype=T16, device=dev)
        ps.append(ops.Gemm(x, w, y, T, N, K, K, N if bk else K, N, bias=None if bk else torch.randn(N, device=dev)))
        a_ops.append(x)
        b_ops.append(w)
    return ps, (False, bk), a_ops, b_ops


def wcase(shapes):
    """one weight-gradient launch: dW [N][K] = dy^T x for every (N, K) of `shapes`, both towers, with the bias-gradient row sums"""
    ps, a_ops, b_ops = [], [], []
    for T in (Tt, Ti):
        for N, K in shapes:
            dy, x = rnd(T, N, scale=0.05), rnd(T, K)
            dw = torch.zeros((N, K), dtype=torch.float32, device=dev)
            ps.append(ops.Gemm(dy, x, dw, N, K, T, N, K, K, rowsum=torch.zeros(N, dtype=torch.float32, device=dev)))
            a_ops.append(dy)
            b_ops.append(x)
    return ps, (True, True), a_ops, b_ops


cases = {"fwd_qkv N2304 K768": case(3 * D, D, False), "fwd_out N768 K768": case(D, D, False), "fwd_ffn1 N3072 K768": case(I, D, False),
         "fwd_ffn2 N768 K3072": case(D, I, False), "dgrad_ffn2 N3072 K768": case(I, D, True), "dgrad_ffn1 N768 K3072": case(D, I, True),
         "dgrad_out N768 K768": case(D, D, True), "dgrad_qkv N768 K2304": case(D, 3 * D, True),
         "wgrad_attn qkv+out": wcase([(3 * D, D), (D, D)]), "wgrad_ffn ffn1+ffn2": wcase([(I, D), (D, I)])}


def once(ps, lay, prep):
    prep()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ops.gemm_grouped(ps, *lay)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main(argv):
    out = None
    if "--out" in argv:
        out = open(argv[argv.index("--out") + 1], "w")
        argv = [a for i, a in enumerate(argv) if a != "--out" and argv[i - 1] != "--out"]
    builds = {a.split("=", 1)[0]: load_build(a.split("=", 1)[1]) for a in argv} or {"package": _lib.load("fp16")}
    _lib.load("fp16")

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    for name, (ps, lay, a_ops, b_ops) in cases.items():
        def hot():
            ops.gemm_grouped(ps, *lay)

        def cold():
            flush.fill_(1.0)

        def b_cold():
            flush.fill_(1.0)
            for x in a_ops:
                x.float().sum()

        def a_cold():
            flush.fill_(1.0)
            for w in b_ops:
                w.float().sum()
        for tag, prep in (("hot", hot), ("all cold", cold), ("B cold", b_cold), ("A cold", a_cold)):
            ts = {b: [] for b in builds}
            for rep in range(REPS):
                order = list(builds) if rep % 2 == 0 else list(builds)[::-1]
                for b in order:
                    _lib._libs["fp16"] = builds[b]
                    ts[b].append(once(ps, lay, prep))
            say(f"{name:24s} {tag:9s} " + " | ".join(f"{b}: {sorted(v)[len(v) // 2]:6.1f} us" for b, v in ts.items()))


if __name__ == "__main__":
    main(sys.argv[1:])
