"""row_dtype="float16" on the CPU: the host twin of the device's float16 rows -- X rounded to float32, scaled in FP64,
rounded to float32 and then to float16 -- is the default estimator's model on those rows, bit for bit."""
import numpy as np
import pytest

import svm355


def _data():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(120, 7)) * [1.0, 50.0, 1e-3, 1.0, 1.0, 1e-13, 1.0] + [0.0, 3.0, 7.0, 0.0, -2.0, 0.0, 0.0]
    X[:, 6] = 0.25  # a constant column and (column 5) one of range < 1e-12: both divide by 1
    X[3, 0] = X[:, 0].min() + 1e-5 * np.ptp(X[:, 0])  # scales to ~1e-5 < 2^-14: a float16 subnormal, kept
    s = X[:, 0] + 0.02 * X[:, 1] + 0.3 * rng.normal(size=120)
    return X, np.where(s > np.median(s), 1, -1).astype(np.int32), np.sin(X[:, 0]) + 0.1 * X[:, 3]


def _rounded_scaled(X):
    X64 = X.astype(np.float32).astype(np.float64)
    mn, rng = X64.min(0), X64.max(0) - X64.min(0)
    rng[rng < 1e-12] = 1.0
    return ((X64 - mn) / rng).astype(np.float32).astype(np.float16).astype(np.float64)


@pytest.mark.parametrize("kind", ["svc", "svr"])
def test_cpu_float16_is_the_default_model_on_the_rounded_rows(kind):
    X, y, z = _data()
    make = (lambda **kw: svm355.SVC(C=10.0, gamma=0.5, device="cpu", **kw)) if kind == "svc" else (
        lambda **kw: svm355.SVR(C=10.0, gamma=0.5, epsilon=0.05, device="cpu", **kw))
    t = y if kind == "svc" else z
    R = _rounded_scaled(X)
    assert 0.0 < R[3, 0] < 2.0**-14
    a, b = make(row_dtype="float16").fit(X, t), make(scale=False).fit(R, t)
    assert a.row_dtype == "float16" and len(a.support_) > 0 and a.b_ == b.b_
    np.testing.assert_array_equal(a.support_, b.support_)
    np.testing.assert_array_equal(a.dual_coef_, b.dual_coef_)
    np.testing.assert_array_equal(a.support_vectors_, R[a.support_])
    X64 = X.astype(np.float32).astype(np.float64)
    np.testing.assert_array_equal(a.scaler_.min_, X64.min(0))
    np.testing.assert_array_equal(a.scaler_.max_, X64.max(0))
