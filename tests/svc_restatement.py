"""The C-SVC solver of include/memehip.h ("SVM"), restated in float64 numpy for the SVC tests (not a test module).

``solve``     libsvm's SMO with second-order working-set selection (Fan, Chen, Lin 2005, WSS2) as the header documents it: per-sample
              bounds, ties to the lowest index, libsvm's two-variable update and its rho.  Written from the paper and the header, not
              from the device code.
``make_case`` the recipe of the fixture: features on a 1/16 grid inside (-1, 1), so that X X^T is exact in f32 and in f64.
``bounds``    C_i = C * class_weight[y_i] * sample_weight_i, as sklearn forms them.
``gradient``  G = Q alpha - e in float64 without the n x n matrix.
"""
import numpy as np

TAU = 1e-12
RUNNING, CONVERGED, MAXITER = 0, 1, 2


def make_case(n, d, sep, seed, n_test=256):
    """(X [n, d], y [n] in {-1, +1}, X_test [n_test, d]), float64 holding multiples of 1/16"""
    mu = sep * np.random.default_rng(1000 + seed).standard_normal(d)
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(n + n_test) < 0.28, 1.0, -1.0)
    X = np.round(16.0 * np.tanh(0.6 * rng.standard_normal((n + n_test, d)) + 0.5 * y[:, None] * mu)) / 16.0
    return X[:n], y[:n], X[n:]


def bounds(y, C=1.0, class_weight=None, sample_weight=None):
    y = np.asarray(y)
    cv = np.full(y.shape[0], float(C))
    if class_weight == "balanced":
        cv *= np.where(y > 0, y.shape[0] / (2.0 * np.sum(y > 0)), y.shape[0] / (2.0 * np.sum(y <= 0)))
    elif class_weight is not None:
        cv *= np.where(y > 0, class_weight[1], class_weight[-1])
    if sample_weight is not None:
        cv *= np.asarray(sample_weight, dtype=np.float64)
    return cv


def gradient(X, y, alpha):
    X = np.asarray(X, dtype=np.float64)
    return y * (X @ (X.T @ (alpha * y))) - 1.0


def _sets(alpha, y, cv):
    pos, below, above = y > 0, alpha < cv, alpha > 0
    return np.where(pos, below, above), np.where(pos, above, below)      # I_up, I_low


def _rho(alpha, G, y, cv):
    up, low = _sets(alpha, y, cv)
    live, yG = cv > 0, y * G
    free = live & up & low
    if free.any():
        return float(yG[free].mean())
    lb = yG[live & ~up & ~free]
    ub = yG[live & up & ~low]
    return float(((ub.min() if ub.size else np.inf) + (lb.max() if lb.size else -np.inf)) / 2.0)


def solve(K, y, cv, tol=1e-3, max_iter=-1):
    """-> dict(alpha, G, rho, n_iter, status, gap)"""
    K = np.asarray(K, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    cv = np.asarray(cv, dtype=np.float64)
    n = y.shape[0]
    alpha, G, kd = np.zeros(n), -np.ones(n), np.diag(K).copy()
    idx = np.arange(n)
    it, status, gap = 0, RUNNING, np.inf
    while True:
        up, low = _sets(alpha, y, cv)
        yG = y * G
        if not up.any() or not low.any():
            status, gap = CONVERGED, 0.0
            break
        cand = idx[up]
        i = int(cand[np.argmax(-yG[up])])                # np.argmax: the first maximum = the lowest index
        gmax, gmax2 = -yG[i], yG[low].max()
        gap = gmax + gmax2
        if not gap >= tol:
            status = CONVERGED
            break
        if 0 <= max_iter <= it:
            status = MAXITER
            break
        b = gmax + yG
        ok = low & (b > 0)
        a = kd[i] + kd - 2.0 * K[i]
        a = np.where(a > 0, a, TAU)
        gain = np.where(ok, b * b / a, -np.inf)
        j = int(np.argmax(gain))
        quad = kd[i] + kd[j] - 2.0 * K[i, j]
        quad = quad if quad > 0 else TAU
        ai, aj, ci, cj = alpha[i], alpha[j], cv[i], cv[j]
        if y[i] != y[j]:
            delta, diff = (-G[i] - G[j]) / quad, ai - aj
            ai, aj = ai + delta, aj + delta
            if diff > 0:
                if aj < 0:
                    aj, ai = 0.0, diff
            elif ai < 0:
                ai, aj = 0.0, -diff
            if diff > ci - cj:
                if ai > ci:
                    ai, aj = ci, ci - diff
            elif aj > cj:
                aj, ai = cj, cj + diff
        else:
            delta, tot = (G[i] - G[j]) / quad, ai + aj
            ai, aj = ai - delta, aj + delta
            if tot > ci:
                if ai > ci:
                    ai, aj = ci, tot - ci
            elif aj < 0:
                aj, ai = 0.0, tot
            if tot > cj:
                if aj > cj:
                    aj, ai = cj, tot - cj
            elif ai < 0:
                ai, aj = 0.0, tot
        G += y * (y[i] * K[i] * (ai - alpha[i]) + y[j] * K[j] * (aj - alpha[j]))
        alpha[i], alpha[j] = ai, aj
        it += 1
    return dict(alpha=alpha, G=G, rho=_rho(alpha, G, y, cv), n_iter=it, status=status, gap=float(gap))


def load_cases(path):
    """tests/golden/svc_cases.npz (tools/gen_svc_golden.py) -> {case: {field: array}} with X, y, X_test decoded to float64"""
    cases = {}
    with np.load(path) as z:
        for key in z.files:
            name, field = key.split("/")
            cases.setdefault(name, {})[field] = z[key]
    for c in cases.values():
        c["X"], c["X_test"], c["y"] = c["X16"] / 16.0, c["Xt16"] / 16.0, c["y"].astype(np.float64)
    return cases


def certificate(X, y, alpha, cv):
    """(worst box violation, |sum alpha y| summed exactly, Gmax - Gmin) of alpha, from G = Q alpha - e in float64"""
    import math
    G = gradient(X, y, alpha)
    up, low = _sets(alpha, y, cv)
    box = max(0.0, float((-alpha).max()), float((alpha - cv).max()))
    gap = float((-y * G)[up].max() - (-y * G)[low].min()) if up.any() and low.any() else 0.0
    return box, abs(math.fsum((alpha * y).tolist())), gap


def support_of(alpha, y):
    """sklearn's support_ and n_support_: the indices with alpha > 0, the negative class first, ascending within a class"""
    sv = np.flatnonzero(alpha > 0)
    neg, pos = sv[y[sv] < 0], sv[y[sv] > 0]
    return np.concatenate([neg, pos]), np.array([neg.size, pos.size])


def alpha_of(support, dual_coef, n):
    """the dual variables behind sklearn's support_ / dual_coef_ (= alpha_i y_i)"""
    a = np.zeros(n)
    a[np.asarray(support)] = np.abs(np.asarray(dual_coef).reshape(-1))
    return a


def same_support(alpha, y, cv, support, support_ref, alpha_ref, margin=1e-5):
    """support (in dual_coef_'s order) against sklearn's.  Left out are the samples that, in either solution, lie within `margin` of 0
    or of their bound WITHOUT being exactly on it: there two runs that stop at the same gap may differ.  A sample exactly at 0 or
    exactly at its bound is unambiguous and is compared.  Returns (equal, samples of either support left out, the per-class counts
    [negative, positive] of the compared samples of each side)."""
    def unclear(a):
        return ((a != 0) & (np.abs(a) <= margin)) | ((a != cv) & (np.abs(a - cv) <= margin))
    out = unclear(np.asarray(alpha)) | unclear(np.asarray(alpha_ref))
    a, b = np.asarray(support), np.asarray(support_ref)
    a, b, left = a[~out[a]], b[~out[b]], int(out[np.union1d(a, b)].sum())
    counts = [[int((y[s] < 0).sum()), int((y[s] > 0).sum())] for s in (a, b)]
    return np.array_equal(a, b), left, counts[0], counts[1]


def decision(X, y, alpha, rho, X_test):
    """f = X_test . ((alpha * y)^T X) - rho in float64"""
    w = (alpha * y) @ np.asarray(X, dtype=np.float64)
    return np.asarray(X_test, dtype=np.float64) @ w - rho
