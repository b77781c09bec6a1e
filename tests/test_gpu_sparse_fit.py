"""SVC and SVR fitted on sparse (CSR) rows through the public interface, checked against numpy on the densified,
x / max scaled rows: the solver's own optimality conditions recomputed from a reference kernel matrix, and the
decision function of sparse queries.  n = 300, d = 500, about 5 % density, working_set = 4 (the smallest the
solver's shape rule takes: 16 candidates for the classifier, 32 for the regression), so a fit is many outer
iterations and the panel's clear-by-rewalk runs every one of them.
"""
import numpy as np
import pytest

import svm355
from svm355.utils.sparse import toarray

pytestmark = pytest.mark.gpu

N, D_FEAT, C, GAMMA, TOL, EPS = 300, 500, 10.0, 0.05, 1e-5, 1e-12


def rows(seed, n):
    rng = np.random.default_rng(seed)
    X = (1.0 - rng.random((n, D_FEAT))) * (rng.random((n, D_FEAT)) < 0.05)
    X[:, :2] = (1.0 - rng.random((n, 2))) * (rng.random((n, 2)) < 0.5)  # the regression's two features, half stored
    X[0, :2] = 0.0
    return X


@pytest.fixture(scope="module")
def data():
    X, Xq = rows(0, N), rows(1, 40)
    rng = np.random.default_rng(2)
    s = X @ rng.normal(size=D_FEAT) + 0.3 * rng.normal(size=N)
    y = np.where(s > np.median(s), 1, -1).astype(np.int32)
    z = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2
    mx = X.max(0)
    mx[mx < 1e-12] = 1.0
    return {"X": X, "Xq": Xq, "y": y, "z": z, "mx": mx, "K": rbf(X / mx, X / mx)}


def rbf(A, B):
    d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A @ B.T
    return np.exp(-GAMMA * np.maximum(d2, 0.0))


@pytest.mark.parametrize("kind", ["svc", "svr"])
def test_fit_is_optimal_and_predicts(data, kind):
    X, K = svm355.CSR.from_dense(data["X"]), data["K"]
    if kind == "svc":
        m = svm355.SVC(C=C, gamma=GAMMA, tol=TOL, device="cuda:0", solver="decomp", working_set=4).fit(X, data["y"])
        alpha, sign = m.alpha_, data["y"].astype(np.float64)
        f = K @ (alpha * sign) - sign
    else:
        m = svm355.SVR(C=C, gamma=GAMMA, tol=TOL, epsilon=0.1, device="cuda:0", working_set=4).fit(X, data["z"])
        alpha, sign = np.concatenate([m.alpha_, m.alpha_star_]), np.repeat([1.0, -1.0], N)
        g = K @ (m.alpha_ - m.alpha_star_) - data["z"]
        f = np.concatenate([g + 0.1, g - 0.1])
    assert m.stop_reason_ == "converged" and m.timings_["rows"] == "csr" and m.timings_["outer_iterations"] > 4
    ulps = C * 2.0**-50  # the pair update clips one variable and moves the other by the same amount: a few ulp of C
    assert alpha.min() >= -ulps and alpha.max() <= C + ulps
    assert abs(np.sum(alpha * sign)) <= 1e-9
    high = ((sign > 0) & (alpha < C - EPS)) | ((sign < 0) & (alpha > EPS))
    low = ((sign > 0) & (alpha > EPS)) | ((sign < 0) & (alpha < C - EPS))
    b_high, b_low = f[high].min(), f[low].max()
    print(f"{kind}: outer={m.timings_['outer_iterations']} nsv={len(m.support_)} b_low - b_high = {b_low - b_high:.3e}")
    assert b_low <= b_high + 2 * TOL + 1e-9  # 1e-9: n C times K's 1e-11, over-estimated
    # sparse queries: against numpy, and against the same model on the densified queries
    Xq = data["Xq"]
    ref = rbf(Xq / data["mx"], (data["X"] / data["mx"])[m.support_]) @ m.dual_coef_ - m.b_
    got = (m.decision_function if kind == "svc" else m.predict)(svm355.CSR.from_dense(Xq))
    dense = (m.decision_function if kind == "svc" else m.predict)(Xq)
    bound = max(len(m.support_), 1) * 1e-11
    print(f"{kind}: max |sparse - ref| = {np.abs(got - ref).max():.3e}, |sparse - dense| = {np.abs(got - dense).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=bound)
    np.testing.assert_allclose(got, dense, rtol=0, atol=bound)
    if kind == "svc":
        sure = np.abs(ref) > bound
        assert np.array_equal(m.predict(svm355.CSR.from_dense(Xq))[sure], np.where(ref > 0, 1, -1)[sure])
    np.testing.assert_allclose(m.scaler_.min_, 0.0)
    np.testing.assert_allclose(m.support_vectors_, (data["X"] / data["mx"])[m.support_], rtol=0, atol=1e-15)


def _break(X, what):
    c = svm355.CSR(X.data.copy(), X.indices.copy(), X.indptr.copy(), X.shape)
    first = int(np.flatnonzero(np.diff(c.indptr) >= 2)[0])  # a row with two entries
    p = int(c.indptr[first])
    if what == "negative":
        c.data[p] = -0.5
    elif what == "unsorted":
        c.indices[[p, p + 1]] = c.indices[[p + 1, p]]
    elif what == "index":
        c.indices[int(c.indptr[first + 1]) - 1] = D_FEAT
    elif what == "positive_min":
        dense = toarray(c)
        dense[:, 3] = 0.5
        c = svm355.CSR.from_dense(dense)
    return c


@pytest.mark.parametrize("what,est,err", [("negative", "SVC", ValueError), ("positive_min", "SVR", ValueError),
                                          ("unsorted", "SVC", ValueError), ("index", "SVR", ValueError),
                                          ("none", "OneClassSVM", TypeError)])
def test_refusals(data, what, est, err):
    X = _break(svm355.CSR.from_dense(data["X"]), what)
    with pytest.raises(err):
        getattr(svm355, est)(device="cuda:0").fit(X, data["y"] if est == "SVC" else data["z"])
