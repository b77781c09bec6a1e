"""SVC / SVR with kernel="precomputed" on the CPU backend: the fits equal the linear-kernel estimators' fits on the rows
that produced the Gram (given that same Gram), the native oracle takes kernel = 6, save / load, and the refusals."""
import numpy as np
import pytest

from svm355 import SVC, SVR, SVMParams
from svm355.ops import cpu as C

from kfun_checks import C as BOX, EPSILON, load_fixture


def grams(X):
    """The two test Grams in numpy float64, symmetrised to the bit: linear (non-unit diagonal) and RBF."""
    lin = X @ X.T
    sq = np.diag(lin)
    rbf = np.exp(-0.5 * (sq[:, None] + sq[None, :] - 2.0 * lin))
    return {"linear": (lin + lin.T) / 2, "rbf": (rbf + rbf.T) / 2}


@pytest.fixture(scope="module")
def fx():
    f = load_fixture()
    return f["X"], f["y"], f["z"], grams(f["X"])


@pytest.mark.parametrize("name", ["linear", "rbf"])
def test_cpu_fits_equal_the_linear_estimators_given_the_same_gram(fx, name, monkeypatch):
    X, y, z, G = fx
    K = G[name]
    svc = SVC(C=BOX, kernel="precomputed", device="cpu").fit(K, y)
    svr = SVR(C=BOX, epsilon=EPSILON, kernel="precomputed", device="cpu").fit(K, z)
    assert svc.scaler_ is None and svc.support_vectors_.shape == (0, 0) and svc.n_fit_ == len(y)
    monkeypatch.setattr(C, "kernel_gram", lambda A, B, p: K)  # the fits' only call
    lsvc = SVC(C=BOX, kernel="linear", device="cpu").fit(X, y)
    lsvr = SVR(C=BOX, epsilon=EPSILON, kernel="linear", device="cpu").fit(X, z)
    for got, want in ((svc, lsvc), (svr, lsvr)):
        assert got.stop_reason_ == "converged" and (got.b_, got.n_iter_) == (want.b_, want.n_iter_)
        np.testing.assert_array_equal(got.support_, want.support_)
        np.testing.assert_array_equal(got.dual_coef_, want.dual_coef_)
    np.testing.assert_array_equal(svc.decision_function(K[:7]), K[:7][:, svc.support_] @ svc.dual_coef_ - svc.b_)
    with pytest.raises(AttributeError):
        svc.coef_


def test_the_native_oracle_takes_kernel_6_with_kernel_1s_bits(fx):
    _, y, z, G = fx
    p1, p6 = SVMParams(C=BOX, kernel="linear"), SVMParams(C=BOX, kernel="precomputed")
    assert p6.to_struct().kernel == 6
    for K in G.values():
        a1, r1, _, _ = C.decomp_train_gram(K, y, p1, inner_wss=2)
        a6, r6, _, _ = C.decomp_train_gram(K, y, p6, inner_wss=2)
        np.testing.assert_array_equal(a1, a6)
        assert (r1.b, r1.iterations) == (r6.b, r6.iterations)
        a1, r1, _, _ = C.decomp_train_gram_svr(K, z, p1, EPSILON, inner_wss=2)
        a6, r6, _, _ = C.decomp_train_gram_svr(K, z, p6, EPSILON, inner_wss=2)
        np.testing.assert_array_equal(a1, a6)
        assert (r1.b, r1.iterations) == (r6.b, r6.iterations)


@pytest.mark.parametrize("cls,target", [(SVC, 1), (SVR, 2)])
def test_save_load_round_trips_on_the_cpu(fx, cls, target, tmp_path):
    K = fx[3]["linear"]
    m = cls(C=BOX, kernel="precomputed", device="cpu").fit(K, fx[target])
    m.save(tmp_path)
    back = cls.load(tmp_path)
    assert back.params.kernel == "precomputed" and back.n_fit_ == K.shape[0]
    np.testing.assert_array_equal(back.predict(K[:40]), m.predict(K[:40]))


def test_constructs_and_refuses(fx):
    _, y, _, G = fx
    K = G["linear"]
    assert SVC(kernel="precomputed").params.precomputed
    with pytest.raises(ValueError):
        SVC(kernel="cosine")
    bad = K.copy()
    bad[3, 5] = np.nextafter(bad[3, 5], np.inf)
    with pytest.raises(ValueError, match=r"K\[3, 5\].*\(K \+ K\.T\) / 2"):
        SVC(kernel="precomputed", device="cpu").fit(bad, y)
    with pytest.raises(ValueError, match="must be a float64 array"):
        SVC(kernel="precomputed", device="cpu").fit(K.astype(np.float32), y)
    with pytest.raises(ValueError, match="square"):
        SVC(kernel="precomputed", device="cpu").fit(K[:, :10], y)
    with pytest.raises(ValueError, match=r"X must be \(m, 300\)"):
        SVC(C=BOX, kernel="precomputed", device="cpu").fit(K, y).decision_function(K[:, :10])
