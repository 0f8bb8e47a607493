"""sklearn.svm.SVC(kernel="linear") on the device: the classifier of the organizers' SVM baselines (baselines/subtask_2a.py,
subtask_2b.py, subtask_2c.py: ``SVC(C=1, kernel='linear', random_state=0)`` over TF-IDF, image and image + text features).

``solve_batch`` is the primitive: P C-SVC problems over ONE Gram matrix, one workgroup each (csrc/svm.hip; the algorithm and its
limits are written down in include/memehip.h, "SVM").  The Gram matrix, ``coef_`` and the decision values come from the exact-f32
``mh_gemm_f32``.  ``SVC`` is the P = 1 case with sklearn's constructor, methods and fitted attributes.  No CPU path.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from . import _lib, fused, ops

F32, F64 = torch.float32, torch.float64
MAX_N = _lib.MH_SVC_MAX_N
MAX_PROBLEMS = _lib.MH_SVC_MAX_PROBLEMS


class ConvergenceWarning(UserWarning):
    """max_iter ended the solver before the stopping tolerance was reached (sklearn.exceptions.ConvergenceWarning's role)."""


def _device_of(X) -> torch.device:
    if not torch.cuda.is_available():
        raise ValueError("memehip.SVC runs on the HIP device only and none is available (there is no CPU fallback)")
    return X.device if isinstance(X, torch.Tensor) and X.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _features(X, what: str = "X") -> torch.Tensor:
    """[n, d] floats of any kind -> the contiguous f32 tensor the kernels read, where the input is (the caller moves it to the device).
    Checked: 2-D, and finite AS f32 -- a float64 feature beyond 3.4e38 is infinity to the device."""
    if not isinstance(X, torch.Tensor):
        X = torch.from_numpy(np.ascontiguousarray(np.asarray(X, dtype=np.float64)))
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1 or not X.is_floating_point():
        raise ValueError(f"{what} must be a non-empty 2-D array of floats, got shape {tuple(X.shape)} of {X.dtype}")
    X = X.detach().to(F32).contiguous()
    if not bool(torch.isfinite(X).all()):
        raise ValueError(f"{what} holds NaN or infinity (as float32)")
    return X


def _effective_max_iter(max_iter: int, n: int) -> int:
    """libsvm's own cap stands in for 'no limit' (svm.cpp Solver::Solve: max(10^7, 100 l)), so no run is unbounded"""
    return int(max_iter) if max_iter >= 0 else max(10_000_000, 100 * n)


def gram(Xd: torch.Tensor) -> torch.Tensor:
    """K = X X^T in exact f32 (mh_gemm_f32, A = B = X) as [n, ldk] with the row pitch rounded up to 64 floats"""
    n, d = Xd.shape
    ldk = (n + 63) // 64 * 64
    K = torch.zeros((n, ldk), dtype=F32, device=Xd.device)
    fused.gemm_f32(Xd, Xd, K, n, n, d, d, d, ldk)
    return K


def solve_batch(X, y, Cv, tol: float = 1e-3, max_iter: int = -1, budget: int = _lib.MH_SVC_LAUNCH_ITERS):
    """P C-SVC problems that share ``X`` [n, d] and the labels ``y`` (+1 / -1) and differ in their per-sample bounds ``Cv`` [P, n]
    (a C grid, class / sample weights; a bound of 0 masks the sample out: fold masks).  One Gram matrix, one launch sequence:
    every launch runs at most ``budget`` iterations per problem and is repeated until every problem has converged or spent
    ``max_iter`` iterations.

    Returns ``(alpha [P, n] f64, rho [P] f64, n_iter [P] int64, status [P] int64)``; alpha and rho on the device, the other two on
    the host.  status: MH_SVC_CONVERGED (1) or MH_SVC_MAXITER (2)."""
    X = _features(X)
    n = X.shape[0]
    if n > MAX_N:
        raise ValueError(f"SVC: n = {n} samples, the device solver holds at most {MAX_N}")
    yv = torch.as_tensor(np.asarray(y.detach().cpu() if isinstance(y, torch.Tensor) else y, dtype=np.float64))
    if yv.shape != (n,) or not bool(((yv == 1) | (yv == -1)).all()):
        raise ValueError("solve_batch: y must hold n labels, each +1 or -1")
    Cv = torch.as_tensor(np.asarray(Cv.detach().cpu() if isinstance(Cv, torch.Tensor) else Cv, dtype=np.float64))
    if Cv.dim() != 2 or Cv.shape[1] != n or not 1 <= Cv.shape[0] <= MAX_PROBLEMS:
        raise ValueError(f"solve_batch: Cv must be [P, n] with 1 <= P <= {MAX_PROBLEMS}, got {tuple(Cv.shape)}")
    if not bool((torch.isfinite(Cv) & (Cv >= 0)).all()):
        raise ValueError("solve_batch: the bounds must be finite and >= 0")
    if not bool((((Cv > 0) & (yv > 0)).any(1) & ((Cv > 0) & (yv < 0)).any(1)).all()):
        raise ValueError("solve_batch: every problem needs a sample of either class with a bound > 0 (rho is undefined without)")
    if not tol > 0:
        raise ValueError("solve_batch: tol must be > 0")
    return _solve(X.to(_device_of(X)), yv, Cv, tol, max_iter, budget)


def _solve(Xd, yv, Cv, tol, max_iter, budget=_lib.MH_SVC_LAUNCH_ITERS):
    """solve_batch behind its validation: Xd f32 [n, d] on the device, yv [n] and Cv [P, n] float64 on the host"""
    dev, (P, n) = Xd.device, Cv.shape
    K = gram(Xd)
    # |K_st| <= sqrt(K_ss K_tt): a finite diagonal is a finite Gram matrix (finite features can still overflow f32 in X X^T)
    if not bool(torch.isfinite(K.diagonal()).all()):
        raise ValueError("X X^T overflows float32: scale the features")
    yd, Cd = yv.to(dev, F32), Cv.to(dev).contiguous()
    alpha, G = torch.empty((P, n), dtype=F64, device=dev), torch.empty((P, n), dtype=F64, device=dev)
    state = torch.empty((P, _lib.MH_SVC_STATE), dtype=F64, device=dev)
    ops.svc_init(K, yd, Cd, alpha, G, state)
    cap, done = _effective_max_iter(max_iter, n), -1.0
    while True:
        ops.svc_solve(K, yd, Cd, alpha, G, state, tol=tol, budget=budget, max_iter=cap)
        st = state.cpu()                                   # the one synchronisation per launch
        if bool((st[:, 0] != _lib.MH_SVC_RUNNING).all()):
            break
        if float(st[:, 1].sum()) <= done:
            raise _lib.MemehipError("mh_svc_solve: a launch made no progress")
        done = float(st[:, 1].sum())
    return alpha, state[:, 3].clone(), st[:, 1].to(torch.int64), st[:, 0].to(torch.int64)


class SVC:
    """``sklearn.svm.SVC`` for ``kernel="linear"`` and two classes, fitted by the device solver.

    ``decision_function`` returns an f32 tensor on the device (> 0 means ``classes_[1]``); the fitted attributes are numpy arrays in
    sklearn's shapes and order.  ``random_state`` is accepted and unused: libsvm's linear C-SVC without probability estimates draws
    nothing."""

    def __init__(self, C=1.0, kernel="linear", tol=1e-3, class_weight=None, max_iter=-1, random_state=None):
        if kernel != "linear":
            raise ValueError(f"memehip.SVC implements kernel='linear' only, got {kernel!r}")
        if not C > 0:
            raise ValueError("C must be > 0")
        if not tol > 0:
            raise ValueError("tol must be > 0")
        if class_weight is not None and class_weight != "balanced" and not isinstance(class_weight, dict):
            raise ValueError("class_weight must be None, 'balanced' or a dict {label: weight}")
        self.C, self.kernel, self.tol, self.class_weight, self.max_iter, self.random_state = C, kernel, tol, class_weight, max_iter, random_state

    def _bounds(self, y01: np.ndarray, sample_weight) -> np.ndarray:
        n = y01.shape[0]
        cw = np.ones(2)
        if isinstance(self.class_weight, str):                       # "balanced": n / (2 * bincount), as sklearn
            cw = n / (2.0 * np.bincount(y01, minlength=2))
        elif self.class_weight is not None:
            unknown = [k for k in self.class_weight if k not in list(self.classes_)]
            if unknown:
                raise ValueError(f"class_weight names labels that are not in y: {unknown}")
            cw = np.array([float(self.class_weight.get(c, 1.0)) for c in self.classes_.tolist()])
        cv = float(self.C) * cw[y01]
        if sample_weight is not None:
            sw = np.asarray(sample_weight, dtype=np.float64)
            if sw.shape != (n,) or not np.isfinite(sw).all() or (sw < 0).any():
                raise ValueError("sample_weight must hold n finite weights >= 0")
            cv = cv * sw
        return cv

    def fit(self, X, y, sample_weight=None):
        X = _features(X)
        n, d = X.shape
        if n > MAX_N:
            raise ValueError(f"SVC: n = {n} samples, the device solver holds at most {MAX_N}")
        labels = np.asarray(y.detach().cpu() if isinstance(y, torch.Tensor) else y)
        if labels.shape != (n,):
            raise ValueError(f"y must hold one label per row of X: {labels.shape} against {n} rows")
        classes, y01 = np.unique(labels, return_inverse=True)
        if classes.shape[0] != 2:
            raise ValueError(f"memehip.SVC separates two classes, y holds {classes.shape[0]}")
        self.classes_ = classes
        cv = self._bounds(y01, sample_weight)
        if not ((cv > 0) & (y01 == 1)).any() or not ((cv > 0) & (y01 == 0)).any():
            raise ValueError("the weights must leave a sample of either class with a bound > 0")
        dev = _device_of(X)
        Xd = X.to(dev)
        ypm = np.where(y01 == 1, 1.0, -1.0)
        alpha, rho, n_iter, status = _solve(Xd, torch.from_numpy(ypm), torch.from_numpy(cv[None, :].copy()), self.tol, self.max_iter)
        a = alpha[0].cpu().numpy()
        sv = np.flatnonzero(a > 0)
        self.support_ = np.concatenate([sv[y01[sv] == 0], sv[y01[sv] == 1]]).astype(np.int32)
        self.n_support_ = np.array([(y01[sv] == 0).sum(), (y01[sv] == 1).sum()], dtype=np.int32)
        self.alpha_ = a                                                    # the dual variables of every sample, float64
        self.dual_coef_ = (a * ypm)[self.support_][None, :]
        self.intercept_ = np.array([-float(rho[0])])
        self.n_iter_ = np.array([int(n_iter[0])], dtype=np.int32)
        self.fit_status_ = int(int(status[0]) == _lib.MH_SVC_MAXITER)
        # coef = (alpha * y)^T X: C[1][d] = A[1][n] . B with B = X as [K = n][N = d]
        ay = torch.from_numpy(a * ypm).to(dev, F32).contiguous()
        self._coef = torch.empty((1, d), dtype=F32, device=dev)
        fused.gemm_f32(ay, Xd, self._coef, 1, d, n, n, d, d, b_kmajor=True)
        self._intercept = torch.tensor([-float(rho[0])], dtype=F32, device=dev)
        self.coef_ = self._coef.cpu().numpy()
        if self.fit_status_:
            warnings.warn(f"Solver terminated early (max_iter={self.max_iter}).  Consider pre-processing your data with StandardScaler "
                          "or MinMaxScaler.", ConvergenceWarning)
        return self

    def decision_function(self, X) -> torch.Tensor:
        if not hasattr(self, "_coef"):
            raise ValueError("this SVC is not fitted yet")
        X = _features(X)
        if X.shape[1] != self._coef.shape[1]:
            raise ValueError(f"X has {X.shape[1]} features, the model was fitted on {self._coef.shape[1]}")
        dev = self._coef.device
        Xd = X.to(dev)
        m, d = Xd.shape
        f = torch.empty((m, 1), dtype=F32, device=dev)
        fused.gemm_f32(Xd, self._coef, f, m, 1, d, d, d, 1, bias=self._intercept)
        return f.view(m)

    def predict(self, X) -> np.ndarray:
        return self.classes_[(self.decision_function(X) > 0).cpu().numpy().astype(np.int64)]
