"""Pairwise-coupling probabilities on the CPU: the host twin ``ops.cpu.ovo_couple`` against plain loops and its
invariants, and ``OneVsOneSVC(device="cpu", cv=)`` against the scikit-learn fixtures, against ``SVC`` at k = 2,
against the uncalibrated fit, through save / load, and its refusals."""
import numpy as np
import pytest

from ovo_checks import FIT, FIXTURES
from ovo_proba_checks import (MIN_PROB, check_fixture, check_invariants, extreme_case, load_fixture, loop_couple,
                              mixed_sweeps_block, pair_probabilities, sigmoid_r)
from svm355 import SVC, OneVsOneSVC
from svm355.ops import cpu as C
from svm355.utils.data import check_folds_multiclass, stratified_folds


# ------------------------------------------------------------------ the host twin
@pytest.mark.parametrize("k", [2, 3, 4, 10, 64])
def test_twin_against_loops(k):
    r = np.concatenate([pair_probabilities(3, k, k), mixed_sweeps_block(k, 4, 50 + k)])
    proba, label, iters = C.ovo_couple(r)
    want, wlabel, witers = loop_couple(r)
    np.testing.assert_array_equal(proba, want)
    np.testing.assert_array_equal(iters, witers)
    np.testing.assert_array_equal(label, wlabel)
    np.testing.assert_array_equal(label, np.argmax(proba, 1))
    assert np.all(iters == 0) if k == 2 else (np.all(iters < max(100, k)) and iters.max() > 0)
    check_invariants(proba, r, k)
    if k == 2:
        np.testing.assert_array_equal(proba, np.stack([r[:, 0], 1.0 - r[:, 0]], 1))


@pytest.mark.parametrize("k", [3, 4])
def test_twin_with_sigmoid_against_loops(k):
    """With (A, B): the loops use math.exp, which is the host libm's exp as the twin's -- bit for bit too."""
    rng = np.random.default_rng(k)
    P = k * (k - 1) // 2
    dec, A, B = 2.0 * rng.normal(size=(6, P)), -rng.uniform(1, 3, P), 0.2 * rng.normal(size=P)
    got, want = C.ovo_couple(dec, A, B), loop_couple(dec, A, B)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    check_invariants(got[0], sigmoid_r(dec, A, B), k)


def test_twin_thread_count_does_not_matter():
    r = pair_probabilities(37, 5, 9)
    one, many = C.ovo_couple(r, n_threads=1), C.ovo_couple(r, n_threads=7)
    for a, b in zip(one, many):
        np.testing.assert_array_equal(a, b)


def test_twin_sweep_counts_differ_within_a_block():
    r = mixed_sweeps_block(10, 8, 3)
    iters = C.ovo_couple(r)[2]
    assert len(set(iters.tolist())) >= 3 and np.all(iters[0::3] == 0) and np.all(iters[1::3] > 0)
    np.testing.assert_array_equal(iters, loop_couple(r)[2])


def test_twin_extreme_decisions_engage_both_clamps():
    dec, A, B = extreme_case(4)
    proba, label, iters = C.ovo_couple(dec, A, B)
    r = sigmoid_r(dec, A, B)
    assert r.min() == MIN_PROB and r.max() == 1.0 - MIN_PROB
    check_invariants(proba, r, 4, iters)
    np.testing.assert_array_equal(proba, loop_couple(dec, A, B)[0])
    # k = 2: the clamped pair probability itself
    p2 = C.ovo_couple(np.array([[800.0], [-800.0]]), np.array([-1.0]), np.array([0.0]))[0]
    np.testing.assert_array_equal(p2, [[1.0 - MIN_PROB, 1.0 - (1.0 - MIN_PROB)], [MIN_PROB, 1.0 - MIN_PROB]])


@pytest.mark.parametrize("k", [2, 3, 10])
def test_twin_nan_row_leaves_its_neighbours_alone(k):
    r = pair_probabilities(5, k, 20 + k)
    clean = C.ovo_couple(r)
    bad = r.copy()
    bad[2, -1] = np.nan
    proba, label, iters = C.ovo_couple(bad)
    assert np.all(np.isnan(proba[2])) if k > 2 else np.isnan(proba[2]).all()
    assert iters[2] == (0 if k == 2 else max(100, k))  # the cap: a NaN never passes the stop test
    keep = [0, 1, 3, 4]
    np.testing.assert_array_equal(proba[keep], clean[0][keep])
    np.testing.assert_array_equal(iters[keep], clean[2][keep])


def test_twin_refuses_bad_shapes():
    with pytest.raises(ValueError):
        C.ovo_couple(np.ones((2, 4)))  # 4 is no k (k - 1) / 2
    with pytest.raises(ValueError):
        C.ovo_couple(np.ones((2, 3)), A=np.ones(3))  # A without B
    with pytest.raises(ValueError):
        C.ovo_couple(np.ones((2, 3)), A=np.ones(2), B=np.ones(2))
    with pytest.raises(ValueError):
        C.ovo_couple(np.ones(3))
    assert C.ovo_couple(np.ones((0, 3)))[0].shape == (0, 3)


# ------------------------------------------------------------------ the folds
def test_check_folds_multiclass():
    cls = np.array([0, 0, 1, 1, 2, 2])
    np.testing.assert_array_equal(check_folds_multiclass([0, 1, 0, 1, 0, 1], cls, 3), [0, 1, 0, 1, 0, 1])
    with pytest.raises(ValueError, match="K >= 2"):
        check_folds_multiclass([0] * 6, cls, 3)
    with pytest.raises(ValueError, match="empty"):
        check_folds_multiclass([0, 2, 0, 2, 0, 2], cls, 3)
    with pytest.raises(ValueError, match="all its rows in fold"):
        check_folds_multiclass([0, 1, 0, 1, 1, 1], cls, 3)
    with pytest.raises(ValueError, match="shape"):
        check_folds_multiclass([0, 1, 0], cls, 3)
    with pytest.raises(ValueError):
        check_folds_multiclass([0, -1, 0, 1, 0, 1], cls, 3)


# ------------------------------------------------------------------ the estimator
@pytest.fixture(scope="module", params=FIXTURES, ids=lambda p: f"n{p[0]}_seed{p[1]}")
def calibrated(request):
    n, seed = request.param
    fx = load_fixture(n, seed)
    return fx, seed, OneVsOneSVC(device="cpu", cv=5, **FIT).fit(fx["X"], fx["labels"], folds=fx["folds"])


def test_fixture_calibration(calibrated):
    fx, seed, m = calibrated
    check_fixture(m, fx, seed)
    assert set(m.platt_status_) == {"converged"}
    p = m.predict_proba(fx["Xt"])
    assert p.shape == (len(fx["Xt"]), len(m.classes_))
    assert np.all(np.abs(p.sum(1) - 1.0) <= 1e-12) and np.all(p > 0)
    assert m.timings_["fold_solves"] > 0 and m.timings_["cv_ms"] > 0 and m.timings_["platt_ms"] > 0


def test_default_folds_are_stratified_by_class_index(calibrated):
    fx, seed, m = calibrated
    cls = np.searchsorted(m.classes_, fx["labels"])
    m2 = OneVsOneSVC(device="cpu", cv=5, cv_seed=seed, **FIT).fit(fx["X"], fx["labels"])
    np.testing.assert_array_equal(m2.cv_folds_, stratified_folds(cls, 5, seed))
    np.testing.assert_array_equal(m2.cv_folds_, fx["folds"])
    np.testing.assert_array_equal(m2.probA_, m.probA_)


def test_cv_decision_layout(calibrated):
    """Column j of a row of class c is its pair (c, o), o = j for j < c else j + 1: every entry is filled, and a
    pair's sigmoid refitted from the two columns that hold it is the stored one."""
    fx, seed, m = calibrated
    k = len(m.classes_)
    cls = np.searchsorted(m.classes_, fx["labels"])
    assert m.cv_decision_.shape == (len(cls), k - 1) and np.all(m.cv_decision_ != 0.0)
    for p, (a, b) in enumerate((a, b) for a in range(k) for b in range(a + 1, k)):
        rows = np.flatnonzero((cls == a) | (cls == b))
        dec = np.where(cls[rows] == a, m.cv_decision_[rows, b - 1], m.cv_decision_[rows, a])
        pl = C.platt_fit(dec, np.where(cls[rows] == a, 1, -1))
        assert (pl.A, pl.B) == (m.probA_[p], m.probB_[p])


def test_calibration_leaves_the_model_alone(calibrated):
    fx, seed, m = calibrated
    plain = OneVsOneSVC(device="cpu", **FIT).fit(fx["X"], fx["labels"])
    for name in ("support_", "n_support_", "dual_coef_", "rho_", "n_iter_", "support_vectors_"):
        np.testing.assert_array_equal(getattr(m, name), getattr(plain, name))
    np.testing.assert_array_equal(m.decision_function(fx["Xt"]), plain.decision_function(fx["Xt"]))
    np.testing.assert_array_equal(m.predict(fx["Xt"]), plain.predict(fx["Xt"]))
    assert plain.probA_ is None and plain.cv_folds_ is None


def test_two_classes_is_svc_probability_bit_for_bit():
    """k = 2 with the same folds: the held-out decisions, (A, B) and P(first class) are
    SVC(device="cpu", probability=True)'s to the bit; proba[:, 0] is the SVC's P(+1) (its column 1)."""
    fx = load_fixture(*FIXTURES[0])
    keep = fx["labels"] != np.unique(fx["labels"])[2]
    X, labels, folds = fx["X"][keep], fx["labels"][keep], fx["folds"][keep]
    lo = labels.min()
    m = OneVsOneSVC(device="cpu", cv=5, **FIT).fit(X, labels, folds=folds)
    s = SVC(device="cpu", probability=True, cv=5, **FIT).fit(X, np.where(labels == lo, 1, -1), folds=folds)
    np.testing.assert_array_equal(m.cv_decision_[:, 0], s.cv_decision_)
    assert (m.probA_[0], m.probB_[0]) == (s.probA_, s.probB_)
    assert m.platt_status_ == [s.platt_.status]
    pm, ps = m.predict_proba(fx["Xt"]), s.predict_proba(fx["Xt"])
    assert MIN_PROB < ps[:, 1].min() and ps[:, 1].max() < 1.0 - MIN_PROB  # the coupling's clamp is not engaged
    np.testing.assert_array_equal(pm[:, 0], ps[:, 1])
    np.testing.assert_array_equal(pm[:, 1], 1.0 - ps[:, 1])


def test_save_load_round_trip(tmp_path, calibrated):
    fx, seed, m = calibrated
    m.save(tmp_path / "cal")
    assert (tmp_path / "cal" / "prob.npz").exists()
    back = OneVsOneSVC.load(tmp_path / "cal")
    assert back.cv == 5
    np.testing.assert_array_equal(back.probA_, m.probA_)
    np.testing.assert_array_equal(back.probB_, m.probB_)
    np.testing.assert_array_equal(back.predict_proba(fx["Xt"]), m.predict_proba(fx["Xt"]))
    np.testing.assert_array_equal(back.predict(fx["Xt"]), m.predict(fx["Xt"]))
    # an uncalibrated model writes exactly the files it always wrote, and loads without probabilities
    plain = OneVsOneSVC(device="cpu", **FIT).fit(fx["X"], fx["labels"])
    plain.save(tmp_path / "plain")
    assert sorted(f.name for f in (tmp_path / "plain").iterdir()) == [
        "dual_coef.npy", "n_support.npy", "ovo.json", "rho.npy", "scaler.npz", "support.npy", "sv_rows.npy"]
    assert "cv" not in (tmp_path / "plain" / "ovo.json").read_text()
    back = OneVsOneSVC.load(tmp_path / "plain")
    assert back.probA_ is None
    with pytest.raises(ValueError, match="calibrated"):
        back.predict_proba(fx["Xt"])


def test_refusals():
    fx = load_fixture(*FIXTURES[0])
    X, labels = fx["X"], fx["labels"]
    with pytest.raises(ValueError, match="cv="):
        OneVsOneSVC(device="cpu", **FIT).fit(X, labels, folds=fx["folds"])  # folds without cv
    for bad in (1, 0, -3, 2.5, True):
        with pytest.raises(ValueError, match="cv must be"):
            OneVsOneSVC(device="cpu", cv=bad)
    cls = np.searchsorted(np.unique(labels), labels)
    confined = fx["folds"].copy()
    confined[cls == 1] = 3  # a class confined to one fold
    with pytest.raises(ValueError, match="all its rows in fold"):
        OneVsOneSVC(device="cpu", cv=5, **FIT).fit(X, labels, folds=confined)
    with pytest.raises(ValueError, match="shape"):
        OneVsOneSVC(device="cpu", cv=5, **FIT).fit(X, labels, folds=fx["folds"][:-1])
    with pytest.raises(ValueError, match="calibrated"):
        OneVsOneSVC(device="cpu", **FIT).fit(X, labels).predict_proba(fx["Xt"])
    with pytest.raises(ValueError, match="does not support.*cv="):
        OneVsOneSVC(probability=True)
