#!/usr/bin/env python3
"""memehip.SVC at the dataset's size: fit at n = 2143, d = 1536 (the train split; ConvNeXt 768 + BERT 768 features).

Synthetic features by the recipe of tests/svc_restatement.make_case, unquantised: y = +1 with probability 0.28,
X = tanh(0.6 N(0,1) + 0.5 y mu), mu = sep N(0,1), for sep in --sep.  With d = 1536 > n / 2 both are separable: at the baselines' C = 1
no alpha reaches its bound (the largest is 0.003 at sep 0.15 and 0.022 at sep 0.05), so the C grid of the batch goes down to where C
binds.  After a
warm-up fit, per sep and as the median of --runs runs, each a host clock around the call that ends in a synchronise:
    gram_ms          K = X X^T through mh_gemm_f32
    fit_ms           SVC.fit (Gram, solver launches, coef_)
    solver_ms        solve_batch minus gram_ms: the launches and their state read-backs
    iterations, us_per_iteration = solver_ms / iterations, launches = the mh_svc_solve calls of that solve_batch, counted
    batch15_ms       ONE solve_batch of P = 15 problems (5 fold masks x C in {0.0003, 0.001, 1}) against singles15_ms, 15 P = 1
                     calls; batch15_at_bound = the alphas at their bound per problem (0 where C does not bind)
    sklearn_ms       sklearn.svm.SVC on this box's host cores (where sklearn is importable), with their count
Prints one JSON line; --out also writes it to a file.

  python tools/svm_bench.py --out profiles/r20_svc.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make(n, d, sep, seed):
    mu = sep * np.random.default_rng(1000 + seed).standard_normal(d)
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(n) < 0.28, 1.0, -1.0)
    return np.tanh(0.6 * rng.standard_normal((n, d)) + 0.5 * y[:, None] * mu), y


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median_ms(fn, runs):
    res = [timed(fn) for _ in range(runs)]
    return statistics.median(r[0] for r in res), res[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2143)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--sep", type=float, nargs="+", default=[0.15, 0.05])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import multimodal_propaganda_meme_classification_amd as pkg
    from multimodal_propaganda_meme_classification_amd import _lib
    from multimodal_propaganda_meme_classification_amd import ops
    svm = pkg.svm
    launches, launch = [0], ops.svc_solve

    def counted(*a, **kw):
        launches[0] += 1
        return launch(*a, **kw)
    ops.svc_solve = counted                                     # svm.solve_batch calls it through the module
    result = dict(n=args.n, d=args.d, device=torch.cuda.get_device_name(0), launch_iterations=_lib.MH_SVC_LAUNCH_ITERS, cases=[])
    for k, sep in enumerate(args.sep):
        X, y = make(args.n, args.d, sep, 20 + k)
        Xd = torch.from_numpy(X).cuda().float()
        ones = np.ones((1, args.n))
        pkg.SVC().fit(Xd, y)                                                         # warm-up
        gram_ms, _ = median_ms(lambda: svm.gram(Xd), args.runs)
        fit_ms, clf = median_ms(lambda: pkg.SVC().fit(Xd, y), args.runs)
        solve_ms, (_, _, n_iter, status) = median_ms(lambda: svm.solve_batch(Xd, y, ones), args.runs)
        launches[0] = 0
        svm.solve_batch(Xd, y, ones)
        n_launches = launches[0]
        iters = int(n_iter[0])
        folds = np.stack([(np.arange(args.n) % 5 != f).astype(np.float64) for f in range(5)])
        Cv = np.concatenate([c * folds for c in (0.0003, 0.001, 1.0)])
        batch_ms, (b_alpha, _, b_iter, b_status) = median_ms(lambda: svm.solve_batch(Xd, y, Cv), args.runs)
        at_bound = ((b_alpha.cpu().numpy() == Cv) & (Cv > 0)).sum(1)
        singles_ms, _ = median_ms(lambda: [svm.solve_batch(Xd, y, Cv[p:p + 1]) for p in range(15)], args.runs)
        case = dict(sep=sep, gram_ms=round(gram_ms, 3), fit_ms=round(fit_ms, 3), solver_ms=round(solve_ms - gram_ms, 3), iterations=iters,
                    us_per_iteration=round((solve_ms - gram_ms) * 1e3 / max(iters, 1), 3),
                    launches=n_launches, converged=bool(int(status[0]) == _lib.MH_SVC_CONVERGED),
                    n_support=int(clf.n_support_.sum()), train_accuracy=round(float((clf.predict(Xd) == y).mean()), 4),
                    batch15_ms=round(batch_ms, 3), singles15_ms=round(singles_ms, 3), batch15_iterations=[int(v) for v in b_iter], batch15_at_bound=[int(v) for v in at_bound],
                    batch15_converged=bool((b_status == _lib.MH_SVC_CONVERGED).all()))
        if not args.no_sklearn:
            try:
                from sklearn.svm import SVC
                ts = []
                for _ in range(args.runs):
                    t0 = time.perf_counter()
                    sk = SVC(C=1, kernel="linear", random_state=0).fit(X, y)
                    ts.append((time.perf_counter() - t0) * 1e3)
                case.update(sklearn_ms=round(statistics.median(ts), 1), sklearn_iterations=int(sk.n_iter_[0]),
                            host_cores=len(os.sched_getaffinity(0)),
                            max_abs_decision_difference=float(np.abs(sk.decision_function(X) - clf.decision_function(Xd).cpu().numpy()).max()))
            except ImportError:
                case.update(sklearn_ms=None)
        result["cases"].append(case)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
