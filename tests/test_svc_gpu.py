"""memehip.SVC / memehip.svm.solve_batch (csrc/svm.hip: mh_svc_init, mh_svc_solve) on the device.

The references are the sklearn fixture tests/golden/svc_cases.npz (tools/gen_svc_golden.py; sklearn is not imported here) and the
float64 certificate of tests/svc_restatement.py, which needs no reference at all: from the returned float64 alpha, on the host,
G = Q alpha - e with K = X X^T (exact for the fixtures' 1/16-grid features) must satisfy the box, the equality constraint and
Gmax - Gmin <= tol + 1e-8.  The allowance is derived: K is exact, alpha and G are float64 on the device, and the device rebuilds
G from n terms of at most 64 C, so its rounding stays below n^2 64 C 2^-53 < 1e-9 at these sizes.

Bars (each measured figure goes to conftest.parity_log as a fraction of its bar):
  tol=1e-3   max|f - f_ref| <= 4 x spread, spread = max|f_sk - f_ref| of sklearn's own two runs: two correct runs that stop at the
             same gap land at different points of the eps-optimal set; a wrong rho or sign costs 0.1 .. 1
  tol=1e-6   max|f - f_ref| <= 8 x the restatement's own deviation from f_ref (in the fixture)
  f32        the device's decision_function / coef_ against float64 from the same alpha: the fmaf-chain bound
             (terms + 1) 2^-24 sum|terms|
Shapes beyond the fixture (certificate only): the solver holds 1, 2, 4, 8 or 16 samples per thread, and keeps alpha in registers up
to 4; n = 2100, 4100 and 8200 reach the three kernels the fixture's n <= 1030 does not.
"""
import ctypes
import functools
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

import svc_restatement as R
from conftest import GOLDEN, parity_log

pytestmark = pytest.mark.gpu

CASES = R.load_cases(os.path.join(GOLDEN, "svc_cases.npz"))
SINGLE = ["n40", "n64", "n257", "n320", "n1030", "n257_sw", "n257_bal"]
BATCH = ["n257_C0.1", "n257_C1", "n257_C10"]
LINE = re.compile(r'^([\w:]+\/.*?\.[\w:]+)\t(propaganda|not_propaganda)\t[\w-]+')     # format_checker/task2.py:20, restated


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import multimodal_propaganda_meme_classification_amd as m
    return m


def _kwargs(name):
    return dict(class_weight="balanced" if name.endswith("_bal") else None), CASES[name].get("sample_weight")


@functools.lru_cache(maxsize=None)
def _fit(name, tol):
    """one device fit per (case, tol), shared by every test"""
    import multimodal_propaganda_meme_classification_amd as m
    c = CASES[name]
    kw, sw = _kwargs(name)
    return m.SVC(C=float(c["C"]), tol=tol, **kw).fit(c["X"], c["y"].astype(np.int64), sample_weight=sw)


@functools.lru_cache(maxsize=None)
def _batch(tol):
    import multimodal_propaganda_meme_classification_amd as m
    c = CASES[BATCH[0]]
    Cv = np.stack([CASES[b]["cv"] for b in BATCH])
    alpha, rho, n_iter, status = m.svm.solve_batch(c["X"], c["y"], Cv, tol=tol)
    return alpha.cpu().numpy(), rho.cpu().numpy(), n_iter.numpy(), status.numpy()


def _solutions(tol):
    """(case name, alpha, rho) of every fixture case: the single fits and every problem of the C batch"""
    for name in SINGLE:
        clf = _fit(name, tol)
        yield name, clf.alpha_, -float(clf.intercept_[0])
    alpha, rho, _, status = _batch(tol)
    assert (status == 1).all()
    for p, name in enumerate(BATCH):
        yield name, alpha[p], float(rho[p])


def _certify(tag, X, y, alpha, cv, C, tol):
    box, eq, gap = R.certificate(X, y, alpha, cv)
    parity_log(f"[svc certificate {tag} tol={tol:g}] box {box:.1e} |sum alpha y| {eq:.2e} (bar {X.shape[0] * C * 2.0 ** -52:.2e}) "
               f"gap {gap:.6e} (bar {tol + 1e-8:.6e})")
    assert alpha.dtype == np.float64 and box == 0.0, (tag, box)
    assert eq <= X.shape[0] * C * 2.0 ** -52, (tag, eq)
    assert gap <= tol + 1e-8, (tag, gap)


@pytest.mark.parametrize("tol", [1e-3, 1e-6])
def test_optimality_certificate(pkg, tol):
    for name, alpha, _ in _solutions(tol):
        c = CASES[name]
        _certify(name, c["X"], c["y"], alpha, c["cv"], float(c["C"]), tol)
        assert np.all(alpha[c["cv"] == 0] == 0.0)                      # a masked sample never moves
    for name in SINGLE:
        assert _fit(name, tol).fit_status_ == 0 and int(_fit(name, tol).n_iter_[0]) > 0


@pytest.mark.parametrize("n", [2100, 4100, 8200])
def test_certificate_on_every_samples_per_thread_kernel(pkg, n):
    """4, 8 and 16 samples per thread (the last two keep alpha out of registers), with a fold mask and two values of C in one batch"""
    X, y, _ = R.make_case(n, 8, 1.0, 100 + n, n_test=1)
    fold = (np.arange(n) % 5 != 0).astype(np.float64)
    Cv = np.stack([np.full(n, 1.0), 0.5 * fold])
    alpha, rho, n_iter, status = pkg.svm.solve_batch(X, y, Cv, tol=1e-3)
    alpha = alpha.cpu().numpy()
    assert (status.numpy() == 1).all() and (n_iter.numpy() > 0).all() and np.isfinite(rho.cpu().numpy()).all()
    for p, C in enumerate((1.0, 0.5)):
        _certify(f"n={n} problem {p} ({int(n_iter[p])} iterations)", X, y, alpha[p], Cv[p], C, 1e-3)
    assert np.all(alpha[1][fold == 0] == 0.0)


def test_agreement_with_sklearn_at_the_default_tolerance(pkg):
    for name, alpha, rho in _solutions(1e-3):
        c = CASES[name]
        dev = float(np.abs(R.decision(c["X"], c["y"], alpha, rho, c["X_test"]) - c["f_ref"]).max())
        parity_log(f"[svc {name} tol=1e-3] max|f - f_ref| = {dev:.3e} = {dev / float(c['spread']):.2f} x sklearn's spread (bar 4; the "
                   f"restatement: {float(c['ratio']):.2f})")
        assert dev <= 4 * float(c["spread"]), (name, dev)


def test_agreement_at_tight_tolerance(pkg):
    for name, alpha, rho in _solutions(1e-6):
        c = CASES[name]
        dev = float(np.abs(R.decision(c["X"], c["y"], alpha, rho, c["X_test"]) - c["f_ref"]).max())
        parity_log(f"[svc {name} tol=1e-6] max|f - f_ref| = {dev:.3e} = {dev / float(c['dev6']):.2f} x the restatement's (bar 8)")
        assert dev <= 8 * float(c["dev6"]), (name, dev)


@pytest.mark.parametrize("name", SINGLE)
def test_device_f32_decision_function_and_coef(pkg, name):
    c, clf = CASES[name], _fit(name, 1e-3)
    X, y, Xt = c["X"], c["y"], c["X_test"]
    n, d = X.shape
    ay = clf.alpha_ * y
    w, b = ay @ X, float(clf.intercept_[0])
    assert clf.coef_.shape == (1, d) and clf.coef_.dtype == np.float32
    coef_bar = (n + 1) * 2.0 ** -24 * (np.abs(ay) @ np.abs(X))
    coef_err = np.abs(clf.coef_[0].astype(np.float64) - w)
    f = clf.decision_function(Xt)
    assert f.is_cuda and f.dtype == torch.float32 and f.shape == (256,)
    f_bar = (d + 1) * 2.0 ** -24 * (np.abs(Xt) @ np.abs(w) + abs(b))
    f_err = np.abs(f.cpu().numpy().astype(np.float64) - (Xt @ w + b))
    parity_log(f"[svc {name} f32] coef_ error / bar {float((coef_err / np.maximum(coef_bar, 1e-300)).max()):.3f}, "
               f"decision_function error / bar {float((f_err / f_bar).max()):.3f}")
    assert np.all(coef_err <= coef_bar) and np.all(f_err <= f_bar)
    # a tensor on the device and a float64 array give the same values
    assert torch.equal(f, clf.decision_function(torch.from_numpy(Xt).cuda().float()))


@pytest.mark.parametrize("name", SINGLE)
def test_predict_and_support_against_sklearn(pkg, name):
    c, clf = CASES[name], _fit(name, 1e-3)
    far = np.abs(c["f_ref"]) > 8 * float(c["spread"])
    assert far.mean() >= 0.95
    assert np.array_equal(clf.classes_, np.array([-1, 1]))
    assert np.array_equal(clf.predict(c["X_test"])[far], np.where(c["predict"] == 1, 1, -1)[far])
    c6 = _fit(name, 1e-6)
    assert c6.dual_coef_.shape == (1, c6.support_.shape[0]) and c6.n_support_.sum() == c6.support_.shape[0]
    assert np.array_equal(c6.dual_coef_[0], (c6.alpha_ * c["y"])[c6.support_]) and np.all(c6.alpha_[c6.support_] > 0)
    support, n_support = R.support_of(c6.alpha_, c["y"])
    assert np.array_equal(c6.support_, support) and np.array_equal(c6.n_support_, n_support)
    ref = R.alpha_of(c["support6"], c["dual_coef6"], c["y"].shape[0])
    same, left_out, counts, counts_ref = R.same_support(c6.alpha_, c["y"], c["cv"], c6.support_, c["support6"], ref)
    parity_log(f"[svc {name} tol=1e-6] support_ and the order of dual_coef_ equal sklearn's: {same}; n_support_ of the compared samples "
               f"{counts} against {counts_ref} ({left_out} samples within 1e-5 of 0 or their bound, not on it, left out of "
               f"{c6.support_.shape[0]})")
    assert same and counts == counts_ref
    if left_out == 0:
        assert np.array_equal(c6.n_support_, c["n_support6"])
    # where both solutions sit exactly on the bound, dual_coef_ is +-C_i on both sides
    on = np.flatnonzero((c6.alpha_ == c["cv"]) & (ref == c["cv"]) & (c["cv"] > 0))
    ours = dict(zip(c6.support_.tolist(), c6.dual_coef_[0].tolist()))
    theirs = dict(zip(c["support6"].tolist(), c["dual_coef6"][0].tolist()))
    assert all(ours[t] == theirs[t] for t in on.tolist())


def test_labels_of_any_kind_and_class_weight_dict(pkg):
    c = CASES["n257_bal"]
    names = np.where(c["y"] > 0, "propaganda", "not_propaganda")
    counts = {"propaganda": int((c["y"] > 0).sum()), "not_propaganda": int((c["y"] < 0).sum())}
    clf = pkg.SVC(class_weight={k: 257 / (2.0 * v) for k, v in counts.items()}).fit(torch.from_numpy(c["X"]), list(names))
    assert list(clf.classes_) == ["not_propaganda", "propaganda"]
    assert np.array_equal(clf.alpha_, _fit("n257_bal", 1e-3).alpha_)
    assert set(clf.predict(c["X_test"])) <= set(clf.classes_)


def test_end_to_end_baseline_tsv(pkg, golden_dir, tmp_path):
    """tiny MultimodalClassifier -> get_features -> dump_features -> run_imgbert_baseline / run_image_baseline -> the TSV"""
    src = json.load(open(os.path.join(golden_dir, "dev_sample12.json"), encoding="utf-8"))
    for split in ("train", "dev"):
        json.dump(src, open(tmp_path / f"{split}.json", "w"))
    df = pkg.read_data(os.path.join(golden_dir, "dev_sample12.json"))
    ds = pkg.MultimodalDataset(df["id"], df["text"], df["image"], [pkg.l2id[v] for v in df["label"]], max_seq_len=32, image_size=32,
                               synthetic_images=True, vocab_size=512)
    cfg = pkg.ModelConfig(text=pkg.TextConfig(vocab_size=512, hidden=128, layers=2, heads=2, intermediate=256, max_position=64),
                          image=pkg.ImageConfig(image_size=32, hidden=128, layers=2, heads=2, intermediate=256), proj=128)
    model = pkg.MultimodalClassifier.from_config(cfg, seed=4).to("cuda")
    img, txt = pkg.get_features(torch.utils.data.DataLoader(ds, batch_size=5), model, "cuda")
    for split in ("train", "dev"):
        pkg.dump_features(str(tmp_path / "features" / f"{split}_feats.json"), img, txt)
    ids = [str(i) for i in df["id"]]
    for run, parts, run_id in ((pkg.run_imgbert_baseline, (img, txt), "imgbert"), (pkg.run_image_baseline, (img,), "image")):
        out = tmp_path / f"{run_id}.tsv"
        run(str(tmp_path), "dev", "train.json", "dev.json", str(out))
        lines = open(out).read().splitlines()
        assert lines[0] == "id\tclass_label\trun_id" and len(lines) == 1 + len(ids)
        assert all(LINE.match(ln) for ln in lines[1:]) and [ln.split("\t")[0] for ln in lines[1:]] == ids
        assert {ln.split("\t")[2] for ln in lines[1:]} == {run_id}
        x = np.array([[v for part in parts for v in part[i]] for i in ids])
        want = pkg.SVC(C=1, kernel="linear", random_state=0).fit(x, list(df["label"])).predict(x)
        assert [ln.split("\t")[1] for ln in lines[1:]] == list(want)


def test_limits_and_status(pkg):
    c = CASES["n257"]
    X, y, cv = c["X"], c["y"], c["cv"]
    with pytest.warns(pkg.svm.ConvergenceWarning):
        clf = pkg.SVC(max_iter=5).fit(X, y)
    assert clf.fit_status_ == 1 and int(clf.n_iter_[0]) == 5
    box, eq, gap = R.certificate(X, y, clf.alpha_, cv)
    assert box == 0.0 and eq <= 257 * 2.0 ** -52 and gap > 1e-3 and np.count_nonzero(clf.alpha_) <= 10
    with pytest.raises(ValueError, match="16384"):
        pkg.SVC().fit(np.zeros((16385, 2)), np.arange(16385) % 2)
    with pytest.raises(ValueError, match="linear"):
        pkg.SVC(kernel="rbf")
    with pytest.raises(ValueError, match="overflows float32"):          # finite features whose Gram matrix is not
        pkg.SVC().fit(1e20 * X, y)
    # a second fit on the same object reuses nothing stale
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        other = CASES["n64"]
        clf.max_iter = -1
        clf.fit(other["X"], other["y"])
    fresh = _fit("n64", 1e-3)
    assert clf.fit_status_ == 0 and np.array_equal(clf.alpha_, fresh.alpha_) and np.array_equal(clf.coef_, fresh.coef_)
    assert np.array_equal(clf.support_, fresh.support_) and np.array_equal(clf.intercept_, fresh.intercept_)
    assert clf.decision_function(other["X_test"]).shape == (256,)


def test_entry_points_init_step_and_resume(pkg):
    """ops.svc_init / ops.svc_solve themselves: the state after init, one iteration per launch, the library's own limit, and a run
    cut into launches of 16 iterations that ends bit for bit where one long launch ends."""
    from multimodal_propaganda_meme_classification_amd import _lib, ops
    c = CASES["n257"]
    n = 257
    Xd = torch.from_numpy(c["X"]).cuda().float()
    K = pkg.svm.gram(Xd)
    assert torch.equal(K[:, :n].double().cpu(), torch.from_numpy(c["X"] @ c["X"].T))          # exact in f32
    yd, Cd = torch.from_numpy(c["y"]).cuda().float(), torch.from_numpy(c["cv"][None]).cuda()
    alpha, G = torch.full((1, n), 7.0, dtype=torch.float64, device="cuda"), torch.zeros((1, n), dtype=torch.float64, device="cuda")
    state = torch.zeros((1, _lib.MH_SVC_STATE), dtype=torch.float64, device="cuda")
    ops.svc_init(K, yd, Cd, alpha, G, state)
    assert float(alpha.abs().max()) == 0.0 and bool((G == -1.0).all())
    assert state[0, :2].tolist() == [float(_lib.MH_SVC_RUNNING), 0.0] and state[0, 2].item() == float("inf")
    ops.svc_solve(K, yd, Cd, alpha, G, state, tol=1e-3, budget=1)
    st = state.cpu()[0].tolist()
    assert st[:2] == [float(_lib.MH_SVC_RUNNING), 1.0] and 1e-3 < st[2] < 4.0 and int((alpha != 0).sum()) == 2
    moved = alpha[0].nonzero().flatten().tolist()
    assert c["y"][moved[0]] != c["y"][moved[1]] and alpha[0, moved[0]].item() == alpha[0, moved[1]].item()      # y^T alpha = 0
    assert float((G.cpu()[0] - torch.from_numpy(R.gradient(c["X"], c["y"], alpha.cpu().numpy()[0]))).abs().max()) < 1e-12
    # the library's own limit, before any pointer is read
    p = ops._svc_problem(K, yd, Cd, alpha, G, state, 1e-3, 1, -1)
    p.n = _lib.MH_SVC_MAX_N + 1
    assert _lib.load().mh_svc_solve(ctypes.byref(p), None) == _lib.MH_ESHAPE == _lib.load().mh_svc_init(ctypes.byref(p), None)
    p.n, p.P = n, _lib.MH_SVC_MAX_PROBLEMS + 1
    assert _lib.load().mh_svc_solve(ctypes.byref(p), None) == _lib.MH_ESHAPE
    # resume
    long_run = pkg.svm.solve_batch(Xd, c["y"], c["cv"][None], tol=1e-6)
    cut = pkg.svm.solve_batch(Xd, c["y"], c["cv"][None], tol=1e-6, budget=16)
    assert int(long_run[2][0]) == int(cut[2][0]) > 16 and torch.equal(long_run[0], cut[0]) and torch.equal(long_run[1], cut[1])
    assert np.array_equal(long_run[0].cpu().numpy()[0], _fit("n257", 1e-6).alpha_)
