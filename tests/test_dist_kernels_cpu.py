"""The laplacian and chi2 kernels on the CPU backend: the host Gram, the estimators, the names, the refusal table."""
import numpy as np
import pytest

from svm355 import SVC, SVR, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C

from dist_checks import KERNELS, kernel_ref, FIXTURE, rows_with_zeros


@pytest.mark.parametrize("d", [1, 17])
@pytest.mark.parametrize("name", list(KERNELS))
def test_host_gram_against_longdouble(name, d):
    X = rows_with_zeros(70, d, d)
    kw = dict(kernel=name, gamma=2.0 / d)
    ref, bound = kernel_ref(X, X[:50], **kw)
    assert np.all(np.abs(C.kernel_gram(X, X[:50], SVMParams(**kw)) - ref) <= bound)  # libm's exp held to the device's figure
    S = C.kernel_gram(X, X, SVMParams(**kw))
    assert np.array_equal(S, S.T) and np.all(np.diag(S) == 1.0)


@pytest.mark.parametrize("cls,target", [(SVC, "y"), (SVR, "z")])
@pytest.mark.parametrize("name", list(KERNELS))
def test_cpu_estimators_fit_and_round_trip(name, cls, target, tmp_path):
    fx = dict(np.load(FIXTURE))
    m = cls(C=1.0, device="cpu", **KERNELS[name]).fit(fx["X"], fx[target])
    m.save(tmp_path)
    back = cls.load(tmp_path)
    assert m.stop_reason_ == "converged" and back.params.kernel == name
    np.testing.assert_array_equal(back.predict(fx["Xq"]), m.predict(fx["Xq"]))


def test_kernel_names_and_domain():
    assert SVMParams(kernel="laplacian").to_struct().kernel == 4 and SVMParams(kernel="chi2").to_struct().kernel == 5
    with pytest.raises(ValueError):
        SVMParams(kernel="cosine")
    X, y = np.eye(4) - 0.5 * np.eye(4)[::-1], np.array([1, -1, 1, -1])
    with pytest.raises(ValueError, match="column 0"):
        SVC(kernel="chi2", scale=False, device="cpu").fit(X, y)
    with pytest.raises(ValueError, match="chi2"):
        SVC(kernel="chi2", device="cpu").fit(np.eye(4), y).predict(np.eye(4) - 1.0)
    with pytest.raises(N.NativeError, match=r"laplacian kernel does not support the distributed solve \(world > 1\)"):
        p = SVMParams(kernel="laplacian")
        C.decomp_train_gram_dist(C.kernel_gram(np.eye(4), np.eye(4), p), y, p, world=2, inner_wss=2)
