"""Platt probabilities and k-fold cross-validation on the CPU: the decomposition oracle's held-out mode
(svm_decomp_train_gram_heldout: label 0 = held out, never selected), the sigmoid fit (svm_platt_fit) against
LIBSVM's own stop rule, the CPU estimator against scikit-learn's fixtures, and the plumbing (folds, persistence,
refusals, predict_proba)."""
import json

import numpy as np
import pytest

from svm355 import SVC, SVMParams
from svm355.ops import cpu as C
from svm355.utils.data import stratified_folds, synthetic_mnist

from probability_checks import (FIXTURES, GRAD_TOL, block0_mask, check_fixture, check_kkt_training_part, load_fixture,
                                platt_cases, platt_gradient, proba_rows)
from svr_checks import rbf_numpy


# ---- the oracle with a mask ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [None, (2.0, 0.5)])
def test_heldout_oracle_with_a_whole_block_held_out(weights):
    """n = 2,000, q = 64: 32 selection blocks of 63 rows; the mask is rows 0..62 plus every 5th row, so block 0 has
    no candidate at all."""
    n, tau = 2000, 1e-5
    tr = synthetic_mnist(n, seed=91)
    X = tr.X / 255.0
    y = np.ascontiguousarray(tr.y, dtype=np.int32)
    mask = block0_mask(n)
    assert mask[:63].all() and set(np.unique(y[~mask])) == {-1, 1}
    p = SVMParams(C=10.0, gamma=0.005, tau=tau, max_iter=10**7)
    if weights:
        p = p.replace(weight_pos=weights[0], weight_neg=weights[1])
    sq = (X * X).sum(1)
    K = np.exp(-p.gamma * np.maximum(sq[:, None] + sq[None, :] - 2.0 * (X @ X.T), 0.0))
    alpha, res, st, f, trace = C.decomp_train_gram_heldout(K, y, mask, p, q=64, trace_cap=400)
    assert res.stop_reason == "converged" and st["outer_iterations"] >= 2
    assert st["working_set"] == 64
    for rec in trace.records():
        W = rec["W"][: rec["m"]]
        assert not mask[W].any()  # a held-out point is never selected
    assert np.all(alpha[mask] == 0.0)
    te = np.flatnonzero(mask)
    ref = K[np.ix_(mask, ~mask)] @ (alpha[~mask] * y[~mask]) - res.b
    assert np.abs((f[te] - res.b) - ref).max() <= 1e-9
    Cp, Cn = (10.0 * weights[0], 10.0 * weights[1]) if weights else (10.0, 10.0)
    check_kkt_training_part(K, y, alpha, res.b, mask, Cp, Cn, tau)


def test_heldout_oracle_agrees_with_a_separate_fit_of_the_training_rows():
    X, y, _ = proba_rows(301, 5)
    p = SVMParams(C=10.0, gamma=0.5, tau=1e-5, max_iter=10**7)
    K = rbf_numpy(X, X, p.gamma)
    folds = stratified_folds(y, 5, 0)
    for j in range(5):
        m = folds == j
        alpha, res, _, f, _ = C.decomp_train_gram_heldout(K, y, m, p)
        assert res.stop_reason == "converged" and np.all(alpha[m] == 0.0)
        a2, r2, _ = C.smo_train(X[~m], y[~m], p)
        ref = K[np.ix_(m, ~m)] @ (a2 * y[~m]) - r2.b
        # both stop inside the same band of tau = 1e-5; at C = 10 and ~100 support vectors a decision value moves by
        # a small multiple of it
        assert np.abs((f[m] - res.b) - ref).max() <= 1e-4


def test_heldout_oracle_refusals(monkeypatch):
    X, y, _ = proba_rows(64, 3)
    K = rbf_numpy(X, X, 0.5)
    m = np.arange(64) % 4 == 0
    with pytest.raises(Exception, match="shrinking"):
        C.decomp_train_gram_heldout(K, y, m, SVMParams(gamma=0.5, shrinking=True))
    monkeypatch.setenv("SVM355_DECOMP_NEWTON", "1")
    with pytest.raises(Exception, match="Newton"):
        C.decomp_train_gram_heldout(K, y, m, SVMParams(gamma=0.5))


# ---- the sigmoid fit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n64_separable", "n300", "n301_30pct", "n5000"])
def test_platt_oracle_meets_libsvms_stop_rule(name):
    dec, y = platt_cases()[name]
    r = C.platt_fit(dec, y)
    g1, g2 = platt_gradient(dec, y, r.A, r.B)
    print(f"{name}: A = {r.A:.6f}, B = {r.B:.6f}, {r.iterations} iterations, gradient ({g1:.2e}, {g2:.2e})")
    assert r.status == "converged" and 1 <= r.iterations < 100
    assert r.A < 0  # a larger decision value is a likelier positive
    assert abs(g1) < GRAD_TOL and abs(g2) < GRAD_TOL


def test_platt_oracle_mask_equals_the_subset():
    dec, y = platt_cases()["n301_30pct"]
    use = np.arange(301) % 3 != 0
    a, b = C.platt_fit(dec, y, use), C.platt_fit(dec[use], y[use])
    assert (a.A, a.B, a.iterations, a.status) == (b.A, b.B, b.iterations, b.status)


def test_platt_oracle_degenerate_inputs_return_a_status():
    dec, y = platt_cases()["n300"]
    for d, lab, prior in ((dec, np.ones(300, dtype=np.int32), np.log(1.0 / 301.0)),
                          (dec, -np.ones(300, dtype=np.int32), np.log(301.0)),
                          (np.full(300, 0.7), y, np.log(((y < 0).sum() + 1.0) / ((y > 0).sum() + 1.0)))):
        r = C.platt_fit(d, lab)
        assert r.status == "degenerate" and r.iterations == 0
        assert r.A == 0.0 and r.B == prior and np.isfinite(r.B)


# ---- scikit-learn fixtures ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_fits():
    out = {}
    for n, seed in FIXTURES:
        g = load_fixture(n, seed)
        out[seed] = (g, SVC(C=g["C"], gamma=g["gamma"], tol=1e-6, max_iter=10**7, device="cpu",
                            probability=True).fit(g["X"], g["y"], folds=g["folds"]))
    return out


@pytest.mark.parametrize("n,seed", FIXTURES)
def test_cpu_estimator_agrees_with_the_scikit_learn_fixture(cpu_fits, n, seed):
    g, m = cpu_fits[seed]
    assert m.stop_reason_ == "converged" and m.platt_.status == "converged"
    np.testing.assert_array_equal(m.scaler_.transform(g["X"]), g["X"])  # the fixture's rows: scaling is the identity
    check_fixture(m, g, seed)
    np.testing.assert_array_equal(m.classes_, [-1, 1])
    assert m.timings_["cv_ms"] > 0 and m.timings_["platt_ms"] > 0


@pytest.mark.parametrize("n,seed", FIXTURES)
def test_decomposition_oracle_masked_folds_agree_with_the_fixture(n, seed):
    """The held-out mode itself against scikit-learn's per-fold fits: k masked solves on one kernel matrix."""
    g = load_fixture(n, seed)
    K = rbf_numpy(g["X"], g["X"], g["gamma"])
    p = SVMParams(C=g["C"], gamma=g["gamma"], tau=1e-6, max_iter=10**7)
    dec = np.zeros(n)
    for j in range(5):
        m = g["folds"] == j
        alpha, res, _, f, _ = C.decomp_train_gram_heldout(K, g["y"], m, p)
        assert res.stop_reason == "converged" and np.all(alpha[m] == 0.0)
        dec[m] = f[m] - res.b
    from probability_checks import FIXTURE_AB_TOL, FIXTURE_DEC_TOL

    err = np.abs(dec - g["cv_decision"]).max()
    r = C.platt_fit(dec, g["y"])
    ab = max(abs(r.A - g["A"]), abs(r.B - g["B"]))
    print(f"seed {seed}: masked folds max |cv decision - fixture| = {err:.3e}, |(A, B) - fixture| = {ab:.3e}")
    assert err <= FIXTURE_DEC_TOL and ab <= FIXTURE_AB_TOL


# ---- plumbing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,pos", [(300, 5, 0.5), (301, 5, 0.3), (103, 7, 0.2), (64, 2, 0.5)])
def test_stratified_folds(n, k, pos):
    rng = np.random.default_rng(n)
    y = np.where(rng.random(n) < pos, 1, -1)
    f = stratified_folds(y, k, seed=3)
    assert f.shape == (n,) and f.dtype.kind == "i"
    assert set(np.unique(f)) == set(range(k))  # every row in exactly one fold: one id each, all ids used
    for c in (-1, 1):
        sizes = np.bincount(f[y == c], minlength=k)
        assert sizes.max() - sizes.min() <= 1
    sizes = np.bincount(f, minlength=k)
    assert sizes.max() - sizes.min() <= 1
    np.testing.assert_array_equal(f, stratified_folds(y, k, seed=3))
    assert np.any(f != stratified_folds(y, k, seed=4))
    with pytest.raises(ValueError, match="k >= 2"):
        stratified_folds(y, 1, 0)


def test_cross_val_decision_and_score(cpu_fits):
    g, m = cpu_fits[31]
    est = SVC(C=g["C"], gamma=g["gamma"], tol=1e-6, max_iter=10**7, device="cpu")
    dec = est.cross_val_decision(g["X"], g["y"], folds=g["folds"])
    np.testing.assert_array_equal(dec, m.cv_decision_)
    acc = est.cross_val_score(g["X"], g["y"], folds=g["folds"])
    assert acc == np.mean(np.where(dec > 0, 1, -1) == g["y"]) and 0.8 < acc < 0.95
    np.testing.assert_array_equal(est.cross_val_decision(g["X"], g["y"], cv=5, seed=31), dec)  # the fixture's folds
    assert not hasattr(est, "alpha_")  # no model of its own
    with pytest.raises(ValueError, match="predict_proba needs"):
        m2 = SVC(C=g["C"], gamma=g["gamma"], device="cpu").fit(g["X"], g["y"])
        m2.predict_proba(g["Xq"])


def test_save_load_round_trip_carries_the_sigmoid(cpu_fits, tmp_path):
    g, m = cpu_fits[32]
    m.save(tmp_path / "with")
    back = SVC.load(tmp_path / "with")
    assert (back.probA_, back.probB_) == (m.probA_, m.probB_)
    np.testing.assert_array_equal(back.predict_proba(g["Xq"]), m.predict_proba(g["Xq"]))
    np.testing.assert_array_equal(back.predict(g["Xq"]), m.predict(g["Xq"]))
    # a model saved before this change: no probA / probB in model.json's meta
    info = json.loads((tmp_path / "with" / "model.json").read_text())
    assert info["meta"]["probA"] == m.probA_
    plain = SVC(C=g["C"], gamma=g["gamma"], device="cpu").fit(g["X"], g["y"])
    plain.save(tmp_path / "without")
    info = json.loads((tmp_path / "without" / "model.json").read_text())
    assert "probA" not in info["meta"] and "probB" not in info["meta"]
    old = SVC.load(tmp_path / "without")
    np.testing.assert_array_equal(old.predict(g["Xq"]), plain.predict(g["Xq"]))
    assert old.probA_ is None
    with pytest.raises(ValueError, match="predict_proba needs"):
        old.predict_proba(g["Xq"])


def test_refusals():
    X, y, _ = proba_rows(80, 2)
    with pytest.raises(ValueError, match="cv >= 2"):
        SVC(probability=True, cv=1, device="cpu")
    with pytest.raises(ValueError, match="warm start"):
        SVC(probability=True, device="cpu").fit(X, y, alpha0=np.zeros(80))
    with pytest.raises(ValueError, match="shrinking"):
        SVC(probability=True, shrinking=True, device="cpu").fit(X, y)
    with pytest.raises(ValueError, match="cv >= 2"):
        SVC(device="cpu").cross_val_decision(X, y, cv=1)
    with pytest.raises(ValueError, match="shrinking"):
        SVC(shrinking=True, device="cpu").cross_val_score(X, y)
    with pytest.raises(ValueError, match="folds="):
        SVC(device="cpu").fit(X, y, folds=np.arange(80) % 5)
    # a fold whose training part lacks a class: every positive row in fold 0
    folds = np.where(y == 1, 0, 1 + np.arange(80) % 3)
    with pytest.raises(ValueError, match="lacks a class"):
        SVC(probability=True, device="cpu").fit(X, y, folds=folds)
    with pytest.raises(ValueError, match="lacks a class"):
        SVC(device="cpu").cross_val_decision(X, y, folds=folds)
    for bad in (np.arange(79) % 5, np.zeros(80, dtype=np.int64), np.arange(80) % 5 - 1,
                np.where(np.arange(80) < 40, 0, 2)):  # a length, one fold, a negative id, an unused id
        with pytest.raises(ValueError):
            SVC(probability=True, device="cpu").fit(X, y, folds=bad)
    # the GPU-only refusals are decided before any device work
    for kw, what in ((dict(solver="smo"), "solver='smo'"), (dict(scale=False), "scale=True")):
        est = SVC(probability=True, device="cuda", **kw)
        with pytest.raises(ValueError, match=what):
            est._check_cv("cuda")


def test_predict_proba_rows_sum_to_one_and_are_monotone(cpu_fits):
    g, m = cpu_fits[31]
    rng = np.random.default_rng(0)
    Xq = rng.random((400, 6))
    dec, pr = m.decision_function(Xq), m.predict_proba(Xq)
    assert pr.shape == (400, 2) and np.all(pr > 0) and np.all(pr < 1)
    np.testing.assert_allclose(pr.sum(1), 1.0, rtol=0, atol=4.5e-16)  # two roundings of values <= 1 and the sum's
    o = np.argsort(dec)
    assert np.all(np.diff(pr[o, 1]) >= 0) and np.all(np.diff(pr[o, 0]) <= 0)  # A < 0: P(+1) rises with the decision
    assert pr[o[-1], 1] > 0.9 and pr[o[0], 1] < 0.1
    np.testing.assert_array_equal(m.predict(Xq), np.where(dec > 0, 1, -1))  # predict stays the decision's sign
    # the overflow-safe form: huge decisions give 0 / 1 without a warning or a NaN
    m2 = SVC(device="cpu")
    m2.probA_, m2.probB_ = -3.0, 0.1
    m2.decision_function = lambda X: np.array([-1e4, -300.0, 0.0, 300.0, 1e4])
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        p2 = m2.predict_proba(None)
    assert np.all(np.isfinite(p2)) and p2[0, 1] == 0.0 and p2[-1, 1] == 1.0
