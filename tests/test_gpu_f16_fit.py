"""SVC and SVR fitted with row_dtype="float16" through the public interface: the solver's optimality conditions
recomputed against the device's own kernel matrix (the float16 block's store epilogue on all rows, which
test_gpu_f16_block_kernel.py ties to numpy), the scaling-and-rounding rule through support_vectors_, the unchanged
FP64 decision path against numpy, float16 host rows, and the refusals.  n = 300, d = 20, working_set = 4: a fit is many
outer iterations."""
import numpy as np
import pytest
import torch

import svm355
from svm355.ops import device as D

pytestmark = pytest.mark.gpu

N, D_FEAT, C, GAMMA, TOL, EPS = 300, 20, 10.0, 0.5, 1e-5, 1e-12


def rows(seed, n):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, D_FEAT)) * np.r_[np.ones(16), 40.0, 1e-6, 1e-13, 0.0] + np.r_[np.zeros(16), 5.0, 2.0, 0.0, 0.25]
    return X  # columns 17..19: a range of ~1e-5 around 2, a range below 1e-12 (divides by 1), a constant


@pytest.fixture(scope="module")
def data():
    X, Xq = rows(0, N), rows(1, 40)
    rng = np.random.default_rng(2)
    s = X[:, :16] @ rng.normal(size=16) + 0.3 * rng.normal(size=N)
    X64 = X.astype(np.float32).astype(np.float64)
    mn, rg = X64.min(0), X64.max(0) - X64.min(0)
    rg[rg < 1e-12] = 1.0
    dev = torch.device("cuda:0")
    Xd = torch.empty((N, D.padded_dim_f16(D_FEAT)), dtype=torch.float16, device=dev)
    D.minmax_scale_f16_(Xd, D_FEAT, src=D.upload_rows_f32(X, dev))
    ids = torch.arange(N, dtype=torch.int32, device=dev)
    K = D.rbf_block_f16(Xd, Xd, GAMMA, ida=ids, idb=ids).cpu().numpy()
    return {"X": X, "Xq": Xq, "y": np.where(s > np.median(s), 1, -1).astype(np.int32),
            "z": np.sin(X[:, 0]) + 0.5 * X[:, 1] ** 2, "mn": mn, "rg": rg, "K": K,
            "Xs": ((X64 - mn) / rg).astype(np.float32).astype(np.float16)}


@pytest.mark.parametrize("kind", ["svc", "svr"])
def test_fit_is_optimal_and_predicts(data, kind):
    X, K = data["X"], data["K"]
    kw = dict(C=C, gamma=GAMMA, tol=TOL, device="cuda:0", working_set=4, row_dtype="float16")
    if kind == "svc":
        m = svm355.SVC(solver="decomp", **kw).fit(X, data["y"])
        alpha, sign = m.alpha_, data["y"].astype(np.float64)
        f = K @ (alpha * sign) - sign
    else:
        m = svm355.SVR(epsilon=0.1, **kw).fit(X, data["z"])
        alpha, sign = np.concatenate([m.alpha_, m.alpha_star_]), np.repeat([1.0, -1.0], N)
        g = K @ (m.alpha_ - m.alpha_star_) - data["z"]
        f = np.concatenate([g + 0.1, g - 0.1])
    assert m.stop_reason_ == "converged" and m.timings_["rows"] == "f16" and m.timings_["outer_iterations"] > 4
    ulps = C * 2.0**-50  # the pair update clips one variable and moves the other by the same amount: a few ulp of C
    assert alpha.min() >= -ulps and alpha.max() <= C + ulps
    assert abs(np.sum(alpha * sign)) <= 1e-9
    high = ((sign > 0) & (alpha < C - EPS)) | ((sign < 0) & (alpha > EPS))
    low = ((sign > 0) & (alpha > EPS)) | ((sign < 0) & (alpha < C - EPS))
    b_high, b_low = f[high].min(), f[low].max()
    print(f"{kind}: outer={m.timings_['outer_iterations']} nsv={len(m.support_)} b_low - b_high = {b_low - b_high:.3e}")
    assert b_low <= b_high + 2 * TOL + 1e-9
    # the scaling and two-step rounding rule, to the bit; the scaler is the ordinary one on the float32 values
    np.testing.assert_array_equal(m.support_vectors_, data["Xs"][m.support_].astype(np.float64))
    np.testing.assert_array_equal(m.scaler_.min_, data["mn"])
    # the FP64 decision path over the widened support vectors
    Q = (data["Xq"] - data["mn"]) / data["rg"]
    S = m.support_vectors_
    d2 = (Q * Q).sum(1)[:, None] + (S * S).sum(1)[None, :] - 2.0 * Q @ S.T
    ref = np.exp(-GAMMA * np.maximum(d2, 0.0)) @ m.dual_coef_ - m.b_
    got = (m.decision_function if kind == "svc" else m.predict)(data["Xq"])
    bound = max(len(m.support_), 1) * 1e-11
    print(f"{kind}: max |decision - ref| = {np.abs(got - ref).max():.3e} (bound {bound:.1e})")
    np.testing.assert_allclose(got, ref, rtol=0, atol=bound)
    if kind == "svc":
        sure = np.abs(ref) > bound
        assert np.array_equal(m.predict(data["Xq"])[sure], np.where(ref > 0, 1, -1)[sure])


def test_float16_host_rows_give_the_float32_host_rows_model(data):
    X16 = data["X"][:, :17].astype(np.float16)  # the columns float16 can hold apart
    kw = dict(C=C, gamma=GAMMA, tol=TOL, device="cuda:0", row_dtype="float16")
    a, b = svm355.SVC(**kw).fit(X16, data["y"]), svm355.SVC(**kw).fit(X16.astype(np.float32), data["y"])
    assert a.timings_["rows"] == "f16" and len(a.support_) > 0 and a.b_ == b.b_
    np.testing.assert_array_equal(a.support_, b.support_)
    np.testing.assert_array_equal(a.dual_coef_, b.dual_coef_)
    np.testing.assert_array_equal(a.support_vectors_, b.support_vectors_)
    np.testing.assert_array_equal(a.scaler_.min_, X16.astype(np.float64).min(0))


@pytest.mark.parametrize("what", ["alpha0", "shrinking", "probability", "cv", "smo", "gram", "kcache", "wss2", "poly",
                                  "noscale", "csr", "weights", "bfloat16", "svr-poly", "svr-noscale", "svr-csr",
                                  "svr-weights", "newton", "svr-newton", "ccache"])
def test_refusals(data, what, monkeypatch):
    X, y, z, kw = data["X"], data["y"], data["z"], dict(device="cuda:0", row_dtype="float16")
    env = {"newton": "SVM355_DECOMP_NEWTON", "svr-newton": "SVM355_DECOMP_NEWTON", "ccache": "SVM355_DECOMP_CCACHE"}
    if what in env:  # the polish: refused by the estimator before the upload; the forced column cache: by the solver
        monkeypatch.setenv(env[what], "1")
    fit = {"alpha0": lambda: svm355.SVC(**kw).fit(X, y, alpha0=np.zeros(N)),
           "shrinking": lambda: svm355.SVC(shrinking=True, **kw).fit(X, y),
           "probability": lambda: svm355.SVC(probability=True, **kw).fit(X, y),
           "cv": lambda: svm355.SVC(**kw).cross_val_decision(X, y),
           "smo": lambda: svm355.SVC(solver="smo", **kw).fit(X, y),
           "gram": lambda: svm355.SVC(gram="fp64", **kw).fit(X, y),
           "kcache": lambda: svm355.SVC(kcache="rows", **kw).fit(X, y),
           "wss2": lambda: svm355.SVC(wss="second", **kw).fit(X, y),
           "poly": lambda: svm355.SVC(kernel="poly", **kw).fit(X, y),
           "noscale": lambda: svm355.SVC(scale=False, **kw).fit(X, y),
           "csr": lambda: svm355.SVC(**kw).fit(svm355.CSR.from_dense(np.abs(X)), y),
           "weights": lambda: svm355.SVC(**kw).fit(X, y, sample_weight=np.ones(N)),
           "bfloat16": lambda: svm355.SVC(device="cuda:0", row_dtype="bfloat16"),
           "svr-poly": lambda: svm355.SVR(kernel="poly", **kw).fit(X, z),
           "svr-noscale": lambda: svm355.SVR(scale=False, **kw).fit(X, z),
           "svr-csr": lambda: svm355.SVR(**kw).fit(svm355.CSR.from_dense(np.abs(X)), z),
           "svr-weights": lambda: svm355.SVR(**kw).fit(X, z, sample_weight=np.ones(N)),
           "newton": lambda: svm355.SVC(**kw).fit(X, y), "svr-newton": lambda: svm355.SVR(**kw).fit(X, z),
           "ccache": lambda: svm355.SVC(**kw).fit(X, y)}[what]
    with pytest.raises(ValueError):
        fit()
