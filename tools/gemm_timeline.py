"""Where a grouped GEMM launch of config 3 spends its time, per workgroup: gemm_kernel's 100-MHz stamps (mh_gemm_set_trace)
{entry, first K stage landed, main loop done, epilogue stores issued} for the four forward shapes and two dgrad shapes at the
benchmark's row counts (2096 live text rows + 6304 image rows)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multimodal_propaganda_meme_classification_amd import ops, _lib  # noqa: E402

dev = torch.device("cuda")
BF16 = torch.bfloat16
Tt, Ti, D, I = int(os.environ.get("TT", "2096")), 6304, 768, 3072


def rnd(*s):
    return (torch.randn(*s, device=dev) * 0.5).to(BF16)


def fwd_group(N, K):
    ps = [ops.Gemm(rnd(T, K), rnd(N, K), torch.empty((T, N), dtype=BF16, device=dev), T, N, K, K, K, N, bias=torch.zeros(N, device=dev))
          for T in (Tt, Ti)]
    return ps, False, False


def dgrad_group(Nout, Kin):
    ps = [ops.Gemm(rnd(T, Nout), rnd(Nout, Kin), torch.empty((T, Kin), dtype=BF16, device=dev), T, Kin, Nout, Nout, Kin, Kin) for T in (Tt, Ti)]
    return ps, False, True


cases = {"fwd qkv": fwd_group(3 * D, D), "fwd out": fwd_group(D, D), "fwd ffn1": fwd_group(I, D), "fwd ffn2": fwd_group(D, I),
         "dgrad ffn2": dgrad_group(D, I), "dgrad qkv": dgrad_group(3 * D, D)}

lib = _lib.load()
buf = torch.zeros(4 * 4096, dtype=torch.int64, device="cuda")
for name, (ps, ak, bk) in cases.items():
    for _ in range(3):
        ops.gemm_grouped(ps, ak, bk)
    torch.cuda.synchronize()
    _lib.check(lib.mh_gemm_set_trace(buf.data_ptr()), "trace")
    buf.zero_()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ops.gemm_grouped(ps, ak, bk)
    e1.record()
    torch.cuda.synchronize()
    _lib.check(lib.mh_gemm_set_trace(None), "trace off")
    t = buf.view(-1, 4).cpu().numpy().astype(np.float64)
    t = t[t[:, 0] > 0]
    t0 = t[:, 0].min()
    us = (t - t0) / 100.0                              # 100 MHz -> microseconds
    fill, loop, epi = us[:, 1] - us[:, 0], us[:, 2] - us[:, 1], us[:, 3] - us[:, 2]
    order = np.argsort(us[:, 0])
    starts = us[order, 0]
    span = us[:, 3].max()
    first_wave = starts[:512].max() if len(starts) >= 512 else starts.max()
    print(f"{name:11s} {len(t):5d} workgroups, event time {e0.elapsed_time(e1) * 1e3:6.1f} us, first entry -> last store {span:6.1f} us | "
          f"fill med {np.median(fill):5.2f} (p90 {np.percentile(fill, 90):5.2f})  main loop med {np.median(loop):5.2f} (p10 {np.percentile(loop, 10):5.2f} p90 {np.percentile(loop, 90):5.2f})  "
          f"epilogue med {np.median(epi):5.2f} (p90 {np.percentile(epi, 90):5.2f}) | first 512 entered by {first_wave:5.2f} us; "
          f"entries at {[round(float(x), 1) for x in np.percentile(starts, [10, 25, 50, 75, 90, 100])]}")
    # busy slots over time: how many workgroups are inside [entry, end] at each microsecond
    grid = np.arange(0, span, 1.0)
    busy = [(int(((us[:, 0] <= g_) & (us[:, 3] > g_)).sum()), int(((us[:, 1] <= g_) & (us[:, 2] > g_)).sum())) for g_ in grid]
    print("            resident / in-main-loop workgroups per us:", " ".join(f"{a}/{b}" for a, b in busy[::3]))
