"""Standalone timings of the memory-bound kernels: LayerNorm forward / backward (single jobs and the grouped image + packed-text launches
of configs 3 and 5, the ConvNeXt shape) and the whole-buffer Adam update (plain and guarded).  Inputs rotate over 24 buffer sets so that
the data is not L2 / Infinity-Cache hot (as in the real step).  One line per case: median and spread (max - min) of 5 timed windows,
microseconds per launch.  MEMEHIP_LIB / MEMEHIP_LIB_F16 select another build of the library for an A/B.
   python tools/ln_probe.py [--dtype bf16] [--tag NAME] [--only ln|adam]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import multimodal_propaganda_meme_classification_amd as pkg
from multimodal_propaganda_meme_classification_amd import ops

dev = torch.device("cuda")
T16 = torch.bfloat16 if "--dtype" in sys.argv and sys.argv[sys.argv.index("--dtype") + 1] == "bf16" else torch.float16
TAG = sys.argv[sys.argv.index("--tag") + 1] if "--tag" in sys.argv else "-"
LIB = pkg._lib.load("bf16" if T16 == torch.bfloat16 else "fp16")
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
NBUF = 24


def t(fn, n=20, windows=5):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(windows):
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / n * 1e3)
    return statistics.median(ts), max(ts) - min(ts)


def report(name, fn, mb, n=20):
    med, spread = t(fn, n)
    print(f"[{TAG}] {name:44s} {med:9.2f} us  spread {spread:6.2f}  ({mb:8.1f} MB, {mb / med:5.2f} TB/s)", flush=True)


def st():
    return torch.cuda.current_stream().cuda_stream


def ln_cases(D, specs, n_part=512, label=""):
    """specs: [(rows, live or None)] = the jobs of one grouped launch"""
    sets = []
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    for _ in range(NBUF):
        fj, bj = (pkg._lib.MhLnFwdJob * len(specs))(), (pkg._lib.MhLnBwdJob * len(specs))()
        keep = []
        for k, (rows, live) in enumerate(specs):
            x, dy, add = (torch.randn(rows, D, device=dev).to(T16) for _ in range(3))
            y = torch.empty(rows, D, device=dev, dtype=T16)
            mean, rstd = torch.zeros(rows, device=dev), torch.ones(rows, device=dev)
            part = torch.empty((2, n_part, D), device=dev)
            rd = None if live is None else torch.tensor([live], dtype=torch.int32, device=dev)
            keep += [x, dy, add, y, mean, rstd, part, rd]
            f, b = fj[k], bj[k]
            f.x, f.gamma, f.beta, f.y, f.mean, f.rstd, f.rows, f.eps = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, 1e-6
            b.dy, b.x, b.gamma, b.mean, b.rstd, b.dx_add, b.dx, b.part = dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), add.data_ptr(), y.data_ptr(), part.data_ptr()
            b.n_part, b.rows = n_part, rows
            if rd is not None:
                f.rows_dev = b.rows_dev = rd.data_ptr()
        sets.append((fj, bj, keep))
    i = [0]

    def fwd():
        fj = sets[i[0] % NBUF][0]
        i[0] += 1
        pkg._lib.check(LIB.mh_layernorm_fwd_grouped(fj, len(specs), D, st()), "fwd")

    def bwd():
        bj = sets[i[0] % NBUF][1]
        i[0] += 1
        pkg._lib.check(LIB.mh_layernorm_bwd_grouped(bj, len(specs), D, st()), "bwd")

    live = sum(r if l is None else l for r, l in specs)
    name = label or "+".join(f"{r}" if l is None else f"{r}(live {l})" for r, l in specs)
    report(f"ln fwd D={D} rows {name}", fwd, live * D * 4 / 1e6)
    report(f"ln bwd D={D} rows {name} n_part {n_part}", bwd, (live * D * 8 + len(specs) * 2 * n_part * D * 4) / 1e6)
    del sets
    torch.cuda.empty_cache()


def adam_cases():
    n, n_shadow = 221_714_692, 171_000_000
    p, m, v, gr = (torch.zeros(n, device=dev) for _ in range(4))
    sh = torch.empty(n_shadow, device=dev, dtype=T16)
    hy = torch.tensor([1e-3, .9, .999, 1e-8, 0., 10., 31.6, 1.], device=dev)
    ov = torch.zeros(1, dtype=torch.int32, device=dev)
    mb = (n * 28 + n_shadow * 2) / 1e6
    report("adam whole buffer, plain", lambda: ops.adam_step(p, m, v, gr, sh, n_shadow, hy), mb, n=5)
    report("adam whole buffer, guarded", lambda: ops.adam_step(p, m, v, gr, sh, n_shadow, hy, overflow=ov, ordinal=1), mb, n=5)
    # one backward slice of the step (a transformer layer's 7.1 M parameters), 24 of them per timed call
    k = 7_087_872
    report("adam 7.1 M-element slices, guarded", lambda: [ops.adam_step(p[j * k:(j + 1) * k], m[j * k:(j + 1) * k], v[j * k:(j + 1) * k], gr[j * k:(j + 1) * k],
                                                                       sh[j * k:(j + 1) * k], k, hy, overflow=ov, ordinal=1) for j in range(24)],
           24 * k * 30 / 1e6, n=3)


if __name__ == "__main__":
    print(f"[{TAG}] library: {LIB._name}", flush=True)
    if ONLY != "adam":
        ln_cases(768, [(4096, None)])
        ln_cases(768, [(6304, None)])
        ln_cases(768, [(6304, None), (4096, 2100)], label="config 3: 6304 + 4096(live 2100)")
        ln_cases(1024, [(18464, None), (8192, 4200)], label="config 5: 18464 + 8192(live 4200)")
        ln_cases(96, [(100352, None)], label="ConvNeXt 100352")
    if ONLY != "ln":
        adam_cases()
