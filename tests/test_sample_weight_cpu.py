"""Sample weights (a box per point) on the CPU: the oracle's box arm against its class-weight arm, the weighted
dual's KKT conditions from the estimators' alpha, the scikit-learn fixture, and the refusals."""
import numpy as np
import pytest

from svm355 import SVC, SVR, SVMParams
from svm355.ops import cpu as C

from sample_weight_checks import BOX, EPSILON, GAMMA, check_kkt, load_fixture, problem, rbf


@pytest.mark.parametrize("inner_wss", [1, 2, 3])
def test_the_box_arm_with_per_class_boxes_is_the_class_weight_arm(inner_wss):
    _, Xs, y, _, _ = problem(128, 1)
    K = rbf(Xs, Xs, GAMMA)
    wp, wn = 3.0, 0.25
    a, r, st, _ = C.decomp_train_gram(K, y, SVMParams(C=BOX, weight_pos=wp, weight_neg=wn), q=16, inner_wss=inner_wss)
    b, rb, sb, _ = C.decomp_train_gram_sw(K, y, np.where(y == 1, wp, wn), SVMParams(C=BOX), q=16, inner_wss=inner_wss)
    np.testing.assert_array_equal(a, b)
    assert (r.b, r.iterations, st["outer_iterations"]) == (rb.b, rb.iterations, sb["outer_iterations"])
    assert r.iterations > 100 and np.count_nonzero(a == BOX * wn)  # the smaller box binds: the weights are not idle


def test_the_pairwise_box_arm_with_per_class_boxes_is_the_class_weight_arm():
    _, Xs, y, _, _ = problem(128, 1)
    a, r, _ = C.smo_train(Xs, y, SVMParams(C=BOX, gamma=GAMMA, weight_pos=3.0, weight_neg=0.25))
    b, rb = C.smo_train_sw(Xs, y, np.where(y == 1, 3.0, 0.25), SVMParams(C=BOX, gamma=GAMMA))
    np.testing.assert_array_equal(a, b)
    assert (r.b, r.iterations) == (rb.b, rb.iterations)


@pytest.mark.parametrize("est", ["svc", "svr"])
def test_weighted_fit_meets_the_kkt_conditions_of_its_own_boxes(est):
    X, Xs, y, z, w = problem(300, 2)
    if est == "svc":
        m = SVC(C=BOX, gamma=GAMMA, device="cpu", class_weight={1: 2.0, -1: 0.5}).fit(X, y, sample_weight=w)
    else:
        m = SVR(C=BOX, gamma=GAMMA, epsilon=EPSILON, device="cpu").fit(X, z, sample_weight=w)
    assert m.stop_reason_ == "converged"
    check_kkt(m, Xs, y if est == "svc" else z, w, m.params.tau)


def test_estimators_match_scikit_learn_within_its_own_tolerance_sensitivity():
    fx = load_fixture()
    kw = dict(C=float(fx["C"]), gamma=float(fx["gamma"]), tol=float(fx["tol"]), device="cpu")
    svc = SVC(**kw).fit(fx["X"], fx["y"], sample_weight=fx["w"])
    svr = SVR(epsilon=float(fx["epsilon"]), **kw).fit(fx["X"], fx["z"], sample_weight=fx["w"])
    for name, got in (("svc", svc.decision_function(fx["Xte"])), ("svr", svr.predict(fx["Xte"]))):
        err = np.abs(got - fx[f"{name}_ref"]).max()
        print(f"{name}: max |dec - sklearn(tol=1e-10)| = {err:.3e}, delta = {float(fx[name + '_delta']):.3e}")
        assert err <= 10 * float(fx[f"{name}_delta"])


@pytest.mark.parametrize("w,msg", [
    (np.ones(63), "shape"), (np.full(64, np.nan), "finite and >= 0"), (-np.ones(64), "finite and >= 0"),
    ("one_class", "leaves a class"), (np.full(64, 1e-13), "not above 2 eps")])
def test_invalid_weights_raise(w, msg):
    X, _, y, _, _ = problem(64, 3)
    if isinstance(w, str):
        w = (y == 1).astype(np.float64)
    with pytest.raises(ValueError, match=msg):
        SVC(C=BOX, device="cpu").fit(X, y, sample_weight=w)


@pytest.mark.parametrize("kw,fit,msg", [
    ({"probability": True}, {}, "probability=True"), ({}, {"alpha0": np.zeros(64)}, r"a warm start \(alpha0\)"),
    ({"row_dtype": "float32"}, {}, "row_dtype='float32'"), ({"kernel": "poly"}, {}, "kernel='poly'"),
    ({"shrinking": True}, {}, "shrinking"), ({"wss": "second"}, {}, "wss='second'"), ({}, {"sparse": True}, "sparse input"),
    ({}, {"cross_val": True}, "cross_val")])
def test_the_estimator_refuses_what_sample_weights_do_not_cover(kw, fit, msg):
    X, _, y, _, w = problem(64, 3)
    m = SVC(device="cpu", **kw)
    with pytest.raises(ValueError, match="sample_weight is not supported with " + msg):
        if fit.pop("cross_val", False):
            m.cross_val_score(X, y, sample_weight=w)
        else:
            if fit.pop("sparse", False):
                X = pytest.importorskip("scipy.sparse").csr_matrix(X)
            m.fit(X, y, sample_weight=w, **fit)
