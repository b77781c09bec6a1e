"""SVC and SVR with the linear kernel fitted on sparse (CSR) rows through the public interface, on
test_gpu_sparse_fit.py's data (n = 300, d = 500, about 5 % density, working_set = 4): the solver's optimality
conditions recomputed from the numpy linear Gram of the scaled densified rows, sparse queries, and coef_.
C = 0.1: at C >= 1 the classes separate and no alpha reaches the box, so the clip would go untested (scikit-learn on
the same rows: SVC 282 support vectors, 163 at the box; SVR 239, 23 at the box).

Decision bound (test_gpu_csr_linear_kernel.py derives it): (nsv + z_i + 4) u S_i + u (|ref_i| + |b|), S_i = sum_c
|q_ic| sum_k |coef_k| |Xs_kc|, z_i the query's stored count.
"""
import numpy as np
import pytest

import svm355
from kfun_checks import U
from test_gpu_sparse_fit import D_FEAT, EPS, N, TOL, rows

pytestmark = pytest.mark.gpu
C, LD = 0.1, np.longdouble


@pytest.fixture(scope="module")
def data():
    X, Xq = rows(0, N), rows(1, 40)
    rng = np.random.default_rng(2)
    s = X @ rng.normal(size=D_FEAT) + 0.3 * rng.normal(size=N)
    mx = X.max(0)
    mx[mx < 1e-12] = 1.0
    return {"X": X, "Xq": Xq, "y": np.where(s > np.median(s), 1, -1).astype(np.int32),
            "z": np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2, "mx": mx, "K": (X / mx) @ (X / mx).T}


def fit(kind, X, data):
    if kind == "svc":
        return svm355.SVC(C=C, kernel="linear", tol=TOL, device="cuda:0", working_set=4).fit(X, data["y"])
    return svm355.SVR(C=C, kernel="linear", tol=TOL, epsilon=0.1, device="cuda:0", working_set=4).fit(X, data["z"])


def check_queries(m, kind, data, dense_too):
    """Sparse queries against longdouble numpy on the model's own support vectors (and the densified queries)."""
    Q, Xs, coef = data["Xq"] / data["mx"], m.support_vectors_, m.dual_coef_
    ref = (Q.astype(LD) @ (coef.astype(LD) @ Xs.astype(LD)) - m.b_).astype(np.float64)
    S = np.abs(Q) @ (np.abs(coef) @ np.abs(Xs))
    bound = (len(coef) + (Q != 0).sum(1) + 4) * U * S + U * (np.abs(ref) + abs(m.b_))
    decide = m.decision_function if kind == "svc" else m.predict
    got = decide(svm355.CSR.from_dense(data["Xq"]))
    print(f"{kind}: max |sparse - ref| = {np.abs(got - ref).max():.3e} (bound {bound.min():.3e} .. {bound.max():.3e})")
    assert np.all(np.abs(got - ref) <= bound)
    if dense_too:
        dense = decide(data["Xq"])
        print(f"{kind}: max |sparse - dense| = {np.abs(got - dense).max():.3e}")
        assert np.all(np.abs(got - dense) <= bound)


@pytest.mark.parametrize("kind", ["svc", "svr"])
def test_fit_is_optimal_and_predicts(data, kind):
    m, K = fit(kind, svm355.CSR.from_dense(data["X"]), data), data["K"]
    if kind == "svc":
        alpha, sign = m.alpha_, data["y"].astype(np.float64)
        f = K @ (alpha * sign) - sign
    else:
        alpha, sign = np.concatenate([m.alpha_, m.alpha_star_]), np.repeat([1.0, -1.0], N)
        g = K @ (m.alpha_ - m.alpha_star_) - data["z"]
        f = np.concatenate([g + 0.1, g - 0.1])
    assert m.stop_reason_ == "converged" and m.timings_["rows"] == "csr"
    ulps = C * 2.0**-50  # the pair update clips one variable and moves the other by the same amount: a few ulp of C
    assert alpha.min() >= -ulps and alpha.max() <= C + ulps
    assert abs(np.sum(alpha * sign)) <= 1e-9
    high = ((sign > 0) & (alpha < C - EPS)) | ((sign < 0) & (alpha > EPS))
    low = ((sign > 0) & (alpha > EPS)) | ((sign < 0) & (alpha < C - EPS))
    b_high, b_low = f[high].min(), f[low].max()
    print(f"{kind}: outer={m.timings_['outer_iterations']} nsv={len(m.support_)} at the box "
          f"{int(np.sum(alpha > C - EPS))} b_low - b_high = {b_low - b_high:.3e}")
    assert np.sum(alpha > C - EPS) > 0  # the clip ran
    assert b_low <= b_high + 2 * TOL + 1e-9  # 1e-9: n C max K u is about 1e-13, over-estimated
    check_queries(m, kind, data, dense_too=True)
    wref = (m.dual_coef_.astype(LD) @ m.support_vectors_.astype(LD)).astype(np.float64)
    wbound = (len(m.dual_coef_) + 2) * U * (np.abs(m.dual_coef_) @ np.abs(m.support_vectors_))
    assert m.coef_.shape == (D_FEAT,) and np.all(np.abs(m.coef_ - wref) <= wbound)


@pytest.mark.parametrize("kind", ["svc", "svr"])
def test_dense_fitted_linear_model_takes_sparse_queries(data, kind):
    check_queries(fit(kind, data["X"], data), kind, data, dense_too=False)


@pytest.mark.parametrize("what", ["sigmoid_fit", "poly_query", "weighted_fit"])
def test_refusals(data, what):
    X = svm355.CSR.from_dense(data["X"])
    with pytest.raises(ValueError):
        if what == "sigmoid_fit":
            svm355.SVC(kernel="sigmoid", device="cuda:0").fit(X, data["y"])
        elif what == "poly_query":
            svm355.SVC(kernel="poly", device="cuda:0").fit(data["X"], data["y"]).decision_function(X)
        else:
            svm355.SVC(kernel="linear", device="cuda:0").fit(X, data["y"], sample_weight=np.ones(N))
