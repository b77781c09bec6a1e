"""One-vs-one multi-class SVC on the CPU: the host twin of the vote kernel (``ops.cpu.ovo_votes``) against loops,
``OneVsOneSVC(device="cpu")`` against the scikit-learn fixtures and LIBSVM's layout, k = 2 against ``SVC``,
persistence and the refusals."""
import numpy as np
import pytest

from svm355 import SVC, OneVsOneSVC
from svm355.ops import cpu as C

from ovo_checks import (FIT, FIXTURES, brute_votes, check_against_fixture, check_structure, exact_case, load_fixture,
                        pairs, tie_wins, vote_bound)


# ------------------------------------------------------------------ the host twin
@pytest.mark.parametrize("k, seg", [(2, [3, 4]), (3, [5, 0, 2]), (4, [0, 3, 1, 6]), (5, [2, 2, 2, 2, 0])])
def test_votes_twin_against_loops(k, seg):
    r = np.random.default_rng(k)
    start = np.concatenate([[0], np.cumsum(seg)])
    S = int(start[-1])
    K = r.uniform(0.0, 1.0, size=(7, S + 1))
    K[:, S] = np.nan                      # a pad column is never read
    coef = r.normal(size=(k - 1, S + 2))
    coef[:, S:] = np.nan
    rho = r.normal(size=k * (k - 1) // 2)
    dec, lab = C.ovo_votes(K, start, coef, rho)
    rdec, rlab = brute_votes(K, start, coef, rho)
    assert dec.shape == rdec.shape and lab.dtype == np.int32
    np.testing.assert_allclose(dec, rdec, rtol=0, atol=1e-13)
    assert np.abs(rdec).min() > 1e-9      # no vote hangs on the summation order
    np.testing.assert_array_equal(lab, rlab)


def test_vote_rules():
    # a 3-cycle: 0 beats 1, 1 beats 2, 2 beats 0 -- one vote each, the lowest index wins
    dec, lab = C.ovo_votes(*exact_case(3, {(0, 1), (1, 2)}))
    np.testing.assert_array_equal(dec, [[1.0, -1.0, 1.0]])
    assert lab[0] == 0
    # a decision of exactly 0.0 votes for b
    K, start, coef, rho = exact_case(2, set())
    coef[:] = 0.0
    dec, lab = C.ovo_votes(K, start, coef, rho)
    assert dec[0, 0] == 0.0 and lab[0] == 1
    # k = 10: classes 3 and 7 both win 8 pairs (7 loses to 3, 3 loses to 5), everybody else fewer
    k = 10
    dec, lab = C.ovo_votes(*exact_case(k, tie_wins()))
    votes = np.zeros(k, dtype=int)
    for p, (a, b) in enumerate(pairs(k)):
        votes[a if dec[0, p] > 0 else b] += 1
    assert votes[3] == votes[7] == votes.max() and (votes == votes.max()).sum() == 2
    assert lab[0] == 3


def test_votes_twin_refuses_bad_shapes():
    with pytest.raises(ValueError):
        C.ovo_votes(np.ones((1, 2)), [0, 1, 2], np.ones((1, 2)), np.zeros(3))  # rho of the wrong length
    with pytest.raises(ValueError):
        C.ovo_votes(np.ones((1, 2)), [0, 2, 1], np.ones((1, 2)), np.zeros(1))  # start descends
    with pytest.raises(ValueError):
        C.ovo_votes(np.ones((1, 2)), [0, 1, 3], np.ones((1, 2)), np.zeros(1))  # a segment past K's columns


# ------------------------------------------------------------------ the fixtures
@pytest.fixture(scope="module", params=FIXTURES, ids=lambda f: f"n{f[0]}_seed{f[1]}")
def fitted(request):
    fx = load_fixture(*request.param)
    return fx, OneVsOneSVC(device="cpu", **FIT).fit(fx["X"], fx["labels"])


def test_fixture_decisions_and_predictions(fitted):
    fx, m = fitted
    check_against_fixture(m, fx)
    assert np.array_equal(m.classes_, np.unique(fx["labels"]))
    assert all(s == "converged" for s in m.stop_reasons_) and len(m.n_iter_) == len(m.rho_)


def test_fixture_structure(fitted):
    fx, m = fitted
    check_structure(m, fx)
    # the union of support vectors is scikit-learn's up to points whose alpha sits in the stop rule's tau band
    assert abs(int(m.n_support_.sum()) - int(fx["n_support"].sum())) <= 0.02 * len(fx["labels"])


def test_fixture_layout_slots(fitted):
    """Row j of dual_coef_ holds, for a support vector of class c, the pair (c, o), o = j for j < c else j + 1:
    rebuilding every pair's decision from these slots alone gives decision_function."""
    fx, m = fitted
    k = len(m.classes_)
    start = np.concatenate([[0], np.cumsum(m.n_support_)])
    Kq = C.rbf_matrix(m.scaler_.transform(fx["Xt"]), m.support_vectors_, m.params.gamma, 1)
    dec = m.decision_function(fx["Xt"])
    for p, (a, b) in enumerate(pairs(k)):
        sa, sb = slice(start[a], start[a + 1]), slice(start[b], start[b + 1])
        ref = Kq[:, sa] @ m.dual_coef_[b - 1, sa] + Kq[:, sb] @ m.dual_coef_[a, sb] - m.rho_[p]
        np.testing.assert_allclose(dec[:, p], ref, rtol=0, atol=1e-12)


# ------------------------------------------------------------------ k = 2
def _two_class():
    fx = load_fixture(*FIXTURES[0])
    keep = fx["labels"] != np.unique(fx["labels"])[2]
    keep_t = fx["labels_t"] != np.unique(fx["labels"])[2]
    return fx["X"][keep], fx["labels"][keep], fx["Xt"][keep_t]


def test_two_classes_model_is_svc_bit_for_bit():
    """k = 2: the one pair is SVC's problem on the labels mapped to +-1 (the lower class +1); the pair rows are
    all rows, so both scale by the same bounds.  alpha y, rho and the support vectors agree bit for bit."""
    X, labels, _ = _two_class()
    lo = labels.min()
    m = OneVsOneSVC(device="cpu", **FIT).fit(X, labels)
    s = SVC(device="cpu", **FIT).fit(X, np.where(labels == lo, 1, -1))
    assert m.rho_[0] == s.b_
    np.testing.assert_array_equal(np.sort(m.support_), s.support_)
    by_id = np.argsort(m.support_)
    np.testing.assert_array_equal(m.dual_coef_[0, by_id], s.alpha_[s.support_] * s.support_labels_)
    np.testing.assert_array_equal(m.scaler_.min_, s.scaler_.min_)
    np.testing.assert_array_equal(m.scaler_.max_, s.scaler_.max_)


def test_two_classes_decision_is_svc_bit_for_bit():
    """k = 2: the single pair's decision values equal SVC(device="cpu")'s bit for bit.

    SVC's CPU decision sums from -b over the support vectors in ascending training-row order, the two classes
    interleaved (svm_decision); OneVsOneSVC(device="cpu") evaluates every pair the same way.  (The host twin
    ``ops.cpu.ovo_votes`` sums class segment by class segment, as the vote kernel does: on this case 129 of its 134
    decision values differ from SVC's in the last bits, by at most 6.44e-15 -- which is why the CPU model does not
    take its decisions from the twin.)"""
    X, labels, Xt = _two_class()
    lo = labels.min()
    m = OneVsOneSVC(device="cpu", **FIT).fit(X, labels)
    s = SVC(device="cpu", **FIT).fit(X, np.where(labels == lo, 1, -1))
    d_m, d_s = m.decision_function(Xt)[:, 0], s.decision_function(Xt)
    np.testing.assert_array_equal(d_m, d_s)
    np.testing.assert_array_equal(m.predict(Xt), np.where(d_s > 0, lo, labels.max()))
    # the twin on the same model: within the two summation orders' bound of it
    start = np.concatenate([[0], np.cumsum(m.n_support_)])
    Kq = C.rbf_matrix(m.scaler_.transform(Xt), m.support_vectors_, m.params.gamma, 1)
    twin, _ = C.ovo_votes(Kq, start, m.dual_coef_, m.rho_)
    assert np.all(np.abs(twin[:, 0] - d_s) <= vote_bound(Kq, start, m.dual_coef_, m.rho_)[:, 0])


# ------------------------------------------------------------------ persistence, refusals
def test_save_load_round_trip(tmp_path):
    fx = load_fixture(*FIXTURES[1])
    m = OneVsOneSVC(device="cpu", **FIT).fit(fx["X"], fx["labels"])
    m.save(tmp_path / "model")
    assert not list((tmp_path / "model").glob("*.pkl"))
    r = OneVsOneSVC.load(tmp_path / "model", device="cpu")
    for name in ("dual_coef_", "rho_", "support_", "n_support_", "classes_", "n_iter_", "intercept_"):
        np.testing.assert_array_equal(getattr(r, name), getattr(m, name), err_msg=name)
    assert r.stop_reasons_ == m.stop_reasons_
    np.testing.assert_array_equal(r.decision_function(fx["Xt"]), m.decision_function(fx["Xt"]))
    np.testing.assert_array_equal(r.predict(fx["Xt"]), m.predict(fx["Xt"]))
    assert r.score(fx["Xt"], fx["labels_t"]) == m.score(fx["Xt"], fx["labels_t"])


def test_load_refuses_another_format(tmp_path):
    fx = load_fixture(*FIXTURES[0])
    m = OneVsOneSVC(device="cpu", **FIT).fit(fx["X"], fx["labels"])
    m.save(tmp_path / "model")
    j = tmp_path / "model" / "ovo.json"
    j.write_text(j.read_text().replace("svm355-ovo-v1", "svm355-ovr-v1"))
    with pytest.raises(ValueError, match="format"):
        OneVsOneSVC.load(tmp_path / "model")


def test_refusals():
    r = np.random.default_rng(0)
    X = r.uniform(size=(130, 4))
    with pytest.raises(ValueError, match="at most 64"):
        OneVsOneSVC(device="cpu").fit(X, np.arange(130) % 65)
    with pytest.raises(ValueError, match="at least 2"):
        OneVsOneSVC(device="cpu").fit(X, np.ones(130, dtype=int))
    with pytest.raises(ValueError, match="no rows"):
        OneVsOneSVC(device="cpu").fit(X, np.arange(130) % 3, classes=[0, 1, 2, 5])
    with pytest.raises(ValueError, match="does not list"):
        OneVsOneSVC(device="cpu").fit(X, np.arange(130) % 3, classes=[0, 1])
    with pytest.raises(ValueError, match="transport"):
        OneVsOneSVC(device="cpu").fit(X, np.arange(130) % 3, transport=object())
    for kw in ({"class_weight": "balanced"}, {"probability": True}, {"solver": "smo"}, {"shrinking": True},
               {"newton": True}, {"warm_start": True}, {"transport": object()}):
        with pytest.raises(ValueError, match="does not support"):
            OneVsOneSVC(**kw)
    with pytest.raises(TypeError):
        OneVsOneSVC(no_such_option=1)
    OneVsOneSVC(class_weight=None, probability=False, solver="decomp")  # the defaults by name are fine


def test_classes_argument_and_label_mapping():
    """Labels that are not 0..k-1, listed out of order: classes_ is sorted and predict returns labels."""
    fx = load_fixture(*FIXTURES[0])
    m = OneVsOneSVC(device="cpu", **FIT).fit(fx["X"], fx["labels"], classes=[7, 1, 4])
    assert m.classes_.tolist() == [1, 4, 7]
    assert set(m.predict(fx["Xt"]).tolist()) <= {1, 4, 7}
    assert m.score(fx["Xt"], fx["labels_t"]) > 0.85
