"""Pairwise-coupling probabilities on the GPU (``OneVsOneSVC(device="cuda:0", cv=)``): the scikit-learn fixtures at
the CPU estimator's bounds, the model against the uncalibrated fit bit for bit, persistence across devices, and
one solve at a time against the default width."""
import numpy as np
import pytest
import torch

from svm355 import OneVsOneSVC

from ovo_checks import FIT, FIXTURES, GRAM_PATHS
from ovo_proba_checks import FIXTURE_TOL, check_fixture, load_fixture

pytestmark = pytest.mark.gpu
MODEL = ("support_", "n_support_", "dual_coef_", "rho_", "n_iter_", "classes_")


@pytest.fixture(scope="module")
def fitted():
    """The three fixtures (uint8 rows, real-valued rows, uint8 rows) and their calibrated GPU models, fitted once."""
    out = {}
    for n, seed in FIXTURES:
        fx = load_fixture(n, seed)
        out[seed] = (fx, OneVsOneSVC(device="cuda:0", cv=5, **FIT).fit(fx["X"], fx["labels"], folds=fx["folds"]))
    return out


@pytest.mark.parametrize("seed", [s for _, s in FIXTURES])
def test_fixture(fitted, seed):
    fx, m = fitted[seed]
    check_fixture(m, fx, seed)
    assert set(m.platt_status_) == {"converged"}
    assert m.timings_["gram_path"] == GRAM_PATHS[seed]
    k = len(m.classes_)
    # every pair meets every fold here: P (K + 0) fold solves beside the P solves of the model
    assert m.timings_["fold_solves"] == 5 * k * (k - 1) // 2
    assert m.timings_["cv_ms"] > 0 and m.timings_["platt_ms"] > 0
    p = m.predict_proba(fx["Xt"])
    assert p.shape == (len(fx["Xt"]), k) and np.all(p > 0) and np.all(np.abs(p.sum(1) - 1.0) <= 1e-12)


@pytest.mark.parametrize("seed", [s for _, s in FIXTURES])
def test_calibration_leaves_the_model_alone(fitted, seed):
    fx, m = fitted[seed]
    plain = OneVsOneSVC(device="cuda:0", **FIT).fit(fx["X"], fx["labels"])
    for name in MODEL:
        np.testing.assert_array_equal(getattr(m, name), getattr(plain, name), err_msg=name)
    np.testing.assert_array_equal(m.decision_function(fx["Xt"]), plain.decision_function(fx["Xt"]))
    np.testing.assert_array_equal(m.predict(fx["Xt"]), plain.predict(fx["Xt"]))
    assert plain.probA_ is None
    with pytest.raises(ValueError, match="calibrated"):
        plain.predict_proba(fx["Xt"])


def test_fp64_rows_of_the_uint8_fixture(fitted):
    """The same bytes as float64 rows quantise into the same integers: the same held-out decisions and sigmoids."""
    fx, m = fitted[41]
    f = OneVsOneSVC(device="cuda:0", cv=5, **FIT).fit(fx["X"].astype(np.float64), fx["labels"], folds=fx["folds"])
    check_fixture(f, fx, 41)
    np.testing.assert_array_equal(f.cv_decision_, m.cv_decision_)
    np.testing.assert_array_equal(f.probA_, m.probA_)


def test_one_solve_at_a_time_gives_the_same_bits(fitted):
    fx, m = fitted[43]
    one = OneVsOneSVC(device="cuda:0", cv=5, concurrent_solves=1, **FIT).fit(fx["X"], fx["labels"], folds=fx["folds"])
    assert one.timings_["concurrent_solves"] == 1 and m.timings_["concurrent_solves"] == 10
    for name in MODEL + ("cv_decision_", "probA_", "probB_"):
        np.testing.assert_array_equal(getattr(one, name), getattr(m, name), err_msg=name)
    assert one.platt_status_ == m.platt_status_


def test_a_fold_without_a_pairs_rows_is_skipped(fitted):
    """Fixture 2's smallest class has 7 rows: with 8 folds dealt by hand so that fold 7 holds rows of classes 0
    and 1 only, the pairs among classes 2 and 3 skip it."""
    fx, _ = fitted[42]
    cls = np.searchsorted(np.unique(fx["labels"]), fx["labels"])
    folds = (fx["folds"] % 5).astype(np.int32)
    big = np.flatnonzero(cls <= 1)
    folds[big[::6]] = 5 + (np.arange(len(big[::6])) % 3)  # folds 5, 6, 7: rows of classes 0 and 1 only
    m = OneVsOneSVC(device="cuda:0", cv=8, **FIT).fit(fx["X"], fx["labels"], folds=folds)
    assert m.timings_["fold_solves"] == 5 * 8 + 1 * 5  # the pair (2, 3) meets folds 0 .. 4 only
    c = OneVsOneSVC(device="cpu", cv=8, **FIT).fit(fx["X"], fx["labels"], folds=folds)
    assert c.timings_["fold_solves"] == m.timings_["fold_solves"]
    assert np.abs(m.cv_decision_ - c.cv_decision_).max() <= FIXTURE_TOL[42][0]
    assert np.all(m.cv_decision_ != 0.0)


@pytest.mark.parametrize("seed", [41, 42])
def test_save_on_the_gpu_load_on_both(fitted, seed, tmp_path):
    fx, m = fitted[seed]
    m.save(tmp_path / "model")
    p = m.predict_proba(fx["Xt"])
    g = OneVsOneSVC.load(tmp_path / "model", device="cuda:0")
    np.testing.assert_array_equal(g.probA_, m.probA_)
    np.testing.assert_array_equal(g.predict_proba(fx["Xt"]), p)
    h = OneVsOneSVC.load(tmp_path / "model", device="cpu")
    assert h._dev_model is None and h.cv == 5
    np.testing.assert_array_equal(h.probB_, m.probB_)
    # the host's decisions differ from the device's in the last bits (test_gpu_ovo.py has their bound); through
    # sigmoids of |A| <= 5 and the coupling that stays far inside the fixture's bound
    assert np.abs(h.predict_proba(fx["Xt"]) - p).max() <= FIXTURE_TOL[seed][2]
    h.save(tmp_path / "again")
    back = OneVsOneSVC.load(tmp_path / "again", device="cuda:0")
    np.testing.assert_array_equal(back.predict_proba(fx["Xt"]), p)


def test_refusals_before_device_work():
    fx = load_fixture(*FIXTURES[0])
    with pytest.raises(ValueError, match="cv="):
        OneVsOneSVC(device="cuda:0", **FIT).fit(fx["X"], fx["labels"], folds=fx["folds"])
    folds = fx["folds"].copy()
    folds[fx["labels"] == fx["labels"][0]] = 2
    with pytest.raises(ValueError, match="all its rows in fold"):
        OneVsOneSVC(device="cuda:0", cv=5, **FIT).fit(fx["X"], fx["labels"], folds=folds)
