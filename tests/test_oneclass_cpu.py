"""One-class SVM on the CPU: the pairwise oracle (``OneClassSVM(device="cpu")``, svm_smo_train_oneclass) and the
decomposition oracle's one-class mode (svm_decomp_train_gram_oneclass) against scikit-learn's fixtures, an
independent KKT check, the start's f, persistence and the refusals."""
import numpy as np
import pytest

from svm355 import SVC, SVR, OneClassSVM, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C

from oneclass_checks import FIXTURE_DEC_TOL, FIXTURES, check_kkt, load_fixture
from svr_checks import rbf_numpy, real_rows


def _start(nu, n):
    full = int(nu * n)
    a = np.zeros(n)
    a[:full] = 1.0
    if full < n:
        a[full] = nu * n - full
    return a


# ---- scikit-learn fixtures --------------------------------------------------------------------------------------
@pytest.mark.parametrize("oracle", ["pairwise", "decomp"])
@pytest.mark.parametrize("n,seed", FIXTURES)
def test_oracles_agree_with_the_scikit_learn_fixture(n, seed, oracle):
    g = load_fixture(n, seed)
    X = g["X"]
    if oracle == "pairwise":
        m = OneClassSVM(nu=g["nu"], gamma=g["gamma"], tol=1e-6, max_iter=10**7, device="cpu").fit(X)
        assert m.stop_reason_ == "converged"
        np.testing.assert_array_equal(m.scaler_.transform(X), X)  # the fixture's rows: scaling is the identity
        dec, rho, alpha = m.decision_function(X), m.rho_, m.alpha_
    else:
        K = rbf_numpy(X, X, g["gamma"])
        alpha, res, st, _ = C.decomp_train_gram_oneclass(K, SVMParams(gamma=g["gamma"], tau=1e-6, max_iter=10**7),
                                                         nu=g["nu"])
        assert res.stop_reason == "converged"
        assert st["start_columns"] == int(g["nu"] * n) + (g["nu"] * n != int(g["nu"] * n))
        dec, rho = K @ alpha - res.b, res.b
    err = np.abs(dec - g["decision"]).max()
    print(f"seed {seed} {oracle}: max |decision - fixture| = {err:.3e}, |rho - fixture| = {abs(rho - g['rho']):.3e} "
          f"(bound {FIXTURE_DEC_TOL:.3e})")
    assert err <= FIXTURE_DEC_TOL
    assert abs(rho - g["rho"]) <= FIXTURE_DEC_TOL
    assert abs(alpha.sum() - g["dual_coef"].sum()) <= 1e-9 * n


# ---- independent KKT check --------------------------------------------------------------------------------------
@pytest.mark.parametrize("oracle", ["pairwise", "decomp"])
@pytest.mark.parametrize("n,nu", [(250, 0.1), (251, 0.5), (250, 0.9)])
def test_kkt_from_an_independent_rbf(oracle, n, nu):
    X, _ = real_rows(n, seed=31)
    p = SVMParams(gamma=0.5, tau=1e-5, max_iter=10**7)
    K = rbf_numpy(X, X, p.gamma)
    if oracle == "pairwise":
        alpha, res = C.smo_train_oneclass(X, p, nu)
    else:
        alpha, res, _, _ = C.decomp_train_gram_oneclass(K, p, nu=nu, q=256)
    assert res.stop_reason == "converged"
    clipped = np.clip(alpha, 0.0, 1.0)
    assert np.abs(alpha - clipped).max() <= 1e-14  # what the clamp removes: a few ulp of the box
    check_kkt(K, clipped, res.b, nu, p.tau)


def test_C_and_class_weights_are_not_read():
    X, _ = real_rows(120, seed=32)
    K = rbf_numpy(X, X, 0.5)
    a1, r1 = C.smo_train_oneclass(X, SVMParams(gamma=0.5), 0.3)
    a2, r2 = C.smo_train_oneclass(X, SVMParams(gamma=0.5, C=3.0, weight_pos=2.0), 0.3)
    np.testing.assert_array_equal(a1, a2)
    assert r1.b == r2.b
    d1 = C.decomp_train_gram_oneclass(K, SVMParams(gamma=0.5), nu=0.3)
    d2 = C.decomp_train_gram_oneclass(K, SVMParams(gamma=0.5, C=3.0, weight_neg=0.5), nu=0.3)
    np.testing.assert_array_equal(d1[0], d2[0])
    assert d1[1].b == d2[1].b


# ---- the start ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64_rows", [False, True])
@pytest.mark.parametrize("n,nu", [(300, 0.2), (301, 0.5), (2050, 1024.5 / 2050)])
def test_first_build_bounds_are_the_starts_f(n, nu, fp64_rows):
    """The first outer iteration's bounds are min f over I_high and max f over I_low of the start's f = K alpha0
    (no -y term, nothing off by one); n = 2,050 at nu n = 1,024.5: the start spans two chunks of 1,024 columns."""
    X, _ = real_rows(n, seed=n)
    p = SVMParams(gamma=0.5, tau=1e-5, max_iter=10**7)
    K = rbf_numpy(X, X, p.gamma)
    a0 = _start(nu, n)
    _, res, st, tr = C.decomp_train_gram_oneclass(K, p, nu=nu, trace_cap=1, fp64_rows=fp64_rows)
    assert st["start_columns"] == int((a0 != 0).sum())
    f0 = K @ a0
    bh, bl = tr.records()[0]["bounds"]
    want_h, want_l = f0[a0 < 1 - p.eps].min(), f0[a0 > p.eps].max()
    assert abs(bh - want_h) <= 1e-9 * abs(want_h) and abs(bl - want_l) <= 1e-9 * abs(want_l)


def test_start_numbers():
    import ctypes

    def start(nu, n):
        full, frac = ctypes.c_int64(-1), ctypes.c_double(-1.0)
        N.check(N.core().svm_oneclass_start(float(nu), n, ctypes.byref(full), ctypes.byref(frac)), "start")
        return full.value, frac.value

    assert start(0.2, 300) == (int(0.2 * 300), 0.2 * 300 - int(0.2 * 300))
    assert start(0.5, 301) == (150, 0.5)
    assert start(0.5, 2048) == (1024, 0.0)
    assert start(1022.5 / 2050, 2050)[0] == 1022


# ---- inference and persistence ------------------------------------------------------------------------------------
def test_decision_predict_and_persistence(tmp_path):
    X, _ = real_rows(200, seed=33)
    Xq, _ = real_rows(80, seed=34, bounds_of=X)
    Xq = np.vstack([Xq, Xq[:5] + 3.0])  # far outside the training range: outliers
    m = OneClassSVM(nu=0.2, gamma=0.5, device="cpu").fit(X)
    assert m.stop_reason_ == "converged"
    ref = rbf_numpy(Xq, X, 0.5) @ m.alpha_ - m.rho_
    dec = m.decision_function(Xq)
    assert np.abs(dec - ref).max() < 1e-10
    pred = m.predict(Xq)
    np.testing.assert_array_equal(pred, np.where(dec > 0, 1, -1))
    assert pred.dtype.kind == "i" and set(np.unique(pred)) == {-1, 1} and np.all(pred[-5:] == -1)
    np.testing.assert_array_equal(m.score_samples(Xq), dec + m.rho_)
    np.testing.assert_allclose(m.score_samples(Xq) - dec, m.rho_, rtol=0, atol=1e-12)  # a rounding of rho + dec
    assert m.b_ == m.rho_ == m.offset_ == -m.intercept_
    np.testing.assert_array_equal(m.dual_coef_, m.alpha_[m.support_])
    np.testing.assert_array_equal(m.support_vectors_, X[m.support_])
    m.save(tmp_path / "m")
    back = OneClassSVM.load(tmp_path / "m")
    np.testing.assert_array_equal(back.decision_function(Xq), dec)
    np.testing.assert_array_equal(back.support_, m.support_)
    assert back.nu == 0.2 and back.rho_ == m.rho_


def test_each_class_loads_its_own_kind_only(tmp_path):
    X, z = real_rows(60, seed=35)
    OneClassSVM(nu=0.3, gamma=0.5, device="cpu").fit(X).save(tmp_path / "oc")
    SVR(gamma=0.5, device="cpu").fit(X, z).save(tmp_path / "svr")
    SVC(gamma=0.5, device="cpu").fit(X, np.where(z > np.median(z), 1, -1).astype(np.int32)).save(tmp_path / "svc")
    for cls, d in ((SVC, "oc"), (SVR, "oc"), (OneClassSVM, "svr"), (OneClassSVM, "svc")):
        with pytest.raises(ValueError, match="holds a"):
            cls.load(tmp_path / d)


# ---- refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", [0.0, 1.0, float("nan"), -0.1, 1.5])
def test_nu_outside_the_open_interval_is_refused(nu):
    with pytest.raises(ValueError, match="nu"):
        OneClassSVM(nu=nu)
    X, _ = real_rows(20, seed=36)
    with pytest.raises(N.NativeError, match="nu"):
        C.smo_train_oneclass(X, SVMParams(gamma=0.5), nu)
    with pytest.raises(N.NativeError, match="nu"):
        C.decomp_train_gram_oneclass(rbf_numpy(X, X, 0.5), SVMParams(gamma=0.5), nu=nu)


def test_input_refusals():
    X, _ = real_rows(20, seed=36)
    with pytest.raises(ValueError, match="at least 2 rows"):
        OneClassSVM(device="cpu").fit(X[:1])
    bad = X.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError):
        OneClassSVM(device="cpu").fit(bad)
    with pytest.raises(ValueError):
        OneClassSVM(device="cpu", scale=False).fit(bad)
    m = OneClassSVM(nu=0.3, gamma=0.5, device="cpu").fit(X)
    with pytest.raises(ValueError, match="like the training rows"):
        m.predict(X[:, :5])
    with pytest.raises(ValueError, match="like the training rows"):
        m.decision_function(X[0])


@pytest.mark.parametrize("p,what", [(SVMParams(shrinking=True), "shrinking")])
def test_decomposition_oracle_refusals(p, what, monkeypatch):
    X, _ = real_rows(40, seed=37)
    K = rbf_numpy(X, X, 0.5)
    with pytest.raises(N.NativeError, match=what):
        C.decomp_train_gram_oneclass(K, p.replace(gamma=0.5), nu=0.3)
    monkeypatch.setenv("SVM355_DECOMP_NEWTON", "1")
    with pytest.raises(N.NativeError, match="Newton"):
        C.decomp_train_gram_oneclass(K, SVMParams(gamma=0.5), nu=0.3)
