#!/usr/bin/env python
"""Writes tests/golden/svc_cases.npz: what sklearn.svm.SVC(kernel="linear") gives on the SVC test cases.  CPU only; needs sklearn.

Per case (keys ``<name>/<field>``):
    X16, y, Xt16        the inputs of tests/svc_restatement.make_case as int8 multiples of 1/16 (X X^T is exact in f32)
    C, cv               the constructor's C and the per-sample bounds C * class_weight * sample_weight
    sample_weight       where the case has one
    f_sk, f_ref         decision_function(X_test) at tol=1e-3 and at tol=1e-7 ;  spread = max|f_sk - f_ref|
    dual_coef, support, n_support, intercept, coef, predict     of the tol=1e-3 fit (predict: 1 = the positive class; support
                                                                counts the rows of X, also where a sample_weight is 0)
    dual_coef6, support6, n_support6                            of a tol=1e-6 fit
    dev6                max|f - f_ref| of the float64 restatement (tests/svc_restatement.solve) at tol=1e-6
    ratio               max|f - f_ref| of the restatement at tol=1e-3, over spread
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svc_restatement as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "svc_cases.npz")

# name, n, d, sep, seed, kwargs
SHAPES = [("n40", 40, 8, 0.6, 11), ("n64", 64, 16, 0.3, 12), ("n257", 257, 48, 0.25, 13), ("n320", 320, 64, 0.1, 14),
          ("n1030", 1030, 32, 0.2, 15)]
BATCH_C = (0.1, 1.0, 10.0)


def case_list():
    cases = [(name, n, d, sep, seed, {}) for name, n, d, sep, seed in SHAPES]
    n, d, sep, seed = SHAPES[2][1:]
    sw = np.random.default_rng(77).choice([0.0, 0.5, 1.0, 2.0], size=n)
    cases.append(("n257_sw", n, d, sep, seed, {"sample_weight": sw}))
    cases.append(("n257_bal", n, d, sep, seed, {"class_weight": "balanced"}))
    for c in BATCH_C:
        cases.append(("n257_C%g" % c, n, d, sep, seed, {"C": c}))
    return cases


def build_cases():
    from sklearn.svm import SVC
    out = {}
    for name, n, d, sep, seed, kw in case_list():
        X, y, Xt = R.make_case(n, d, sep, seed)
        C, sw, cw = kw.get("C", 1.0), kw.get("sample_weight"), kw.get("class_weight")
        fits = {}
        for tol in (1e-3, 1e-6, 1e-7):
            fits[tol] = SVC(C=C, kernel="linear", tol=tol, class_weight=cw, random_state=0).fit(X, y.astype(np.int64), sample_weight=sw)
        sk, s6, ref = fits[1e-3], fits[1e-6], fits[1e-7]
        f_sk, f_ref = sk.decision_function(Xt), ref.decision_function(Xt)
        cv = R.bounds(y, C, cw, sw)
        K = X @ X.T
        dev = {}
        for tol in (1e-3, 1e-6):
            r = R.solve(K, y, cv, tol)
            dev[tol] = float(np.abs(R.decision(X, y, r["alpha"], r["rho"], Xt) - f_ref).max())
        spread = float(np.abs(f_sk - f_ref).max())
        # sklearn drops the samples of weight 0 before libsvm sees them and reports support_ in that reduced numbering: put it back
        keep = np.flatnonzero(cv > 0)
        rec = dict(X16=np.round(X * 16).astype(np.int8), y=y.astype(np.int8), Xt16=np.round(Xt * 16).astype(np.int8),
                   C=np.float64(C), cv=cv, f_sk=f_sk, f_ref=f_ref, spread=np.float64(spread),
                   dual_coef=sk.dual_coef_, support=keep[sk.support_].astype(np.int32), n_support=sk.n_support_.astype(np.int32),
                   intercept=sk.intercept_, coef=sk.coef_, predict=(sk.predict(Xt) > 0).astype(np.int8),
                   dual_coef6=s6.dual_coef_, support6=keep[s6.support_].astype(np.int32), n_support6=s6.n_support_.astype(np.int32),
                   dev6=np.float64(dev[1e-6]), ratio=np.float64(dev[1e-3] / spread))
        if sw is not None:
            rec["sample_weight"] = sw
        for k, v in rec.items():
            out[f"{name}/{k}"] = np.asarray(v)
    return out


def main():
    cases = build_cases()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **cases)
    for name in sorted({k.split("/")[0] for k in cases}):
        print(f"{name:10s} spread {float(cases[name + '/spread']):.3e}  restatement/spread {float(cases[name + '/ratio']):.2f}  "
              f"dev6 {float(cases[name + '/dev6']):.3e}  nSV {int(cases[name + '/n_support'].sum())}")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
