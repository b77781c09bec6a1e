"""nu-SVC and nu-SVR on the CPU oracle of the decomposition solver's nu modes (csrc/core/decomp_cpu.cpp): the KKT
conditions from a NumPy FP64 RBF matrix, the equivalence with the existing classifier, the estimators' device="cpu"
backend, and the refusals by their table wording (csrc/include/decomp_mode.h)."""
import numpy as np
import pytest

from svm355 import SVC, NuSVC, NuSVR, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C

from nusvm_checks import SHAPES, SVC_EQUIV_TOL, kkt_nusvc, kkt_nusvr, nu_feasible, nusvc_case
from svr_checks import rbf_numpy, real_rows

GAMMA, TAU = 0.5, 1e-5
P = SVMParams(gamma=GAMMA, tau=TAU, max_iter=10**7, n_threads=8)


@pytest.mark.parametrize("n,q", SHAPES)
@pytest.mark.parametrize("kind,nu", [("mixed", 0.4), ("sorted", 0.4), ("skew", 0.3)])
def test_nusvc_oracle_meets_kkt(n, q, kind, nu):
    X, y = nusvc_case(n, seed=n, kind=kind)
    assert nu_feasible(y, nu) and not nu_feasible(y, 1.0 if kind == "skew" else 1.01)
    if kind == "sorted":
        assert np.all(y[: n // 3] == 1)  # the first selection blocks hold one class only
    K = rbf_numpy(X, X, GAMMA)
    alpha, res, st, (r, rho), _ = C.decomp_train_gram_nusvc(K, y, P, nu=nu, q=q)
    assert res.stop_reason == "converged" and r > 0 and res.b == rho / r
    assert st["working_set"] == {300: 1024, 1537: 256}[n]
    kkt_nusvc(K, y, alpha, r, rho, nu, TAU)


@pytest.mark.parametrize("n,q", SHAPES)
def test_nusvr_oracle_meets_kkt(n, q):
    X, z = real_rows(n, seed=n + 1)
    K = rbf_numpy(X, X, GAMMA)
    alpha2, res, st, (r, rho), _ = C.decomp_train_gram_nusvr(K, z, P.replace(C=2.0), nu=0.3, q=q)
    assert res.stop_reason == "converged" and res.b == rho and r < 0  # the tube -r is positive
    kkt_nusvr(K, z, alpha2, 2.0, r, rho, 0.3, TAU)


def test_nusvc_equals_svc_at_c_one_over_r():
    """NuSVC gives r_; SVC(C = 1 / r_) solves the same problem.  The measured difference is what SVC_EQUIV_TOL is
    ten times of."""
    X, y = nusvc_case(300, seed=7)
    Xq, _ = real_rows(200, seed=8, bounds_of=X)
    kw = dict(gamma=GAMMA, tol=TAU, device="cpu", max_iter=10**7)
    nu = NuSVC(nu=0.4, **kw).fit(X, y)
    assert nu.stop_reason_ == "converged" and nu.r_ > 0 and nu.intercept_ == -nu.rho_ / nu.r_
    svc = SVC(C=1.0 / nu.r_, **kw).fit(X, y)
    diff = np.abs(nu.decision_function(Xq) - svc.decision_function(Xq)).max()
    print(f"max |NuSVC - SVC(1 / r)| decision on held-out rows = {diff:.3e} (bound {SVC_EQUIV_TOL:.3e})")
    assert diff <= SVC_EQUIV_TOL
    np.testing.assert_array_equal(nu.predict(Xq), np.where(nu.decision_function(Xq) > 0, 1, -1))
    free = (nu.alpha_ * nu.r_ > 1e-9) & (nu.alpha_ * nu.r_ < 1 - 1e-9)
    np.testing.assert_allclose(nu.decision_function(X)[free], y[free], rtol=0, atol=2 * TAU / nu.r_)


def test_nusvr_estimator_on_the_cpu(tmp_path):
    X, z = real_rows(300, seed=3)
    m = NuSVR(nu=0.3, C=2.0, gamma=GAMMA, tol=TAU, device="cpu", max_iter=10**7).fit(X, z)
    assert m.stop_reason_ == "converged" and m.epsilon_ > 0 and m.score(X, z) > 0.8
    ref = rbf_numpy(X, X[m.support_], GAMMA) @ m.dual_coef_ + m.intercept_
    assert np.abs(m.predict(X) - ref).max() < 1e-10
    m.save(tmp_path / "m")
    back = NuSVR.load(tmp_path / "m")
    np.testing.assert_array_equal(back.predict(X), m.predict(X))
    assert back.epsilon_ == m.epsilon_
    with pytest.raises(ValueError, match="nusvr"):
        NuSVC.load(tmp_path / "m")


REFUSED = [
    (dict(nu=0.0), {}, "nu must be in (0, 1]"),
    (dict(nu=1.5), {}, "nu must be in (0, 1]"),
    (dict(nu=float("nan")), {}, "nu must be in (0, 1]"),
    (dict(nu=0.3), dict(shrinking=True), "solve does not support shrinking"),
    (dict(nu=0.3), dict(weight_pos=2.0), "solve does not support class weights"),
    (dict(nu=0.3), "newton", "solve does not support the Newton polish (SVM355_DECOMP_NEWTON)"),
]


@pytest.mark.parametrize("kind", ["nusvc", "nusvr"])
@pytest.mark.parametrize("args,params,phrase", REFUSED)
def test_refusals(kind, args, params, phrase, monkeypatch):
    X, z = real_rows(64, seed=11)
    y = np.where(np.arange(64) % 2 == 0, 1, -1).astype(np.int32)
    K = rbf_numpy(X, X, GAMMA)
    if params == "newton":
        monkeypatch.setenv("SVM355_DECOMP_NEWTON", "1")
        params = {}
    solve = C.decomp_train_gram_nusvc if kind == "nusvc" else C.decomp_train_gram_nusvr
    with pytest.raises(N.NativeError) as ei:
        solve(K, y if kind == "nusvc" else z, SVMParams(gamma=GAMMA, **params), **args)
    assert phrase in str(ei.value) and f"svm_decomp_train_gram_{kind}" in str(ei.value)
    if "does not support" in phrase:
        assert ("nu-SVC" if kind == "nusvc" else "nu-SVR") in str(ei.value)


def test_infeasible_nu_and_the_point_cap():
    """(A warm start and world > 1 are rows of the table that no nu entry can express: they take neither.)"""
    X, z = real_rows(64, seed=11)
    y = np.where(np.arange(64) % 4 == 0, 1, -1).astype(np.int32)  # 16 : 48, nu_max = 0.5
    K = rbf_numpy(X, X, GAMMA)
    with pytest.raises(N.NativeError, match="specified nu is infeasible"):
        C.decomp_train_gram_nusvc(K, y, SVMParams(gamma=GAMMA), nu=0.51)
    assert C.decomp_train_gram_nusvc(K, y, SVMParams(gamma=GAMMA), nu=0.5)[1].stop_reason == "converged"
    with pytest.raises(ValueError, match="specified nu is infeasible"):
        NuSVC(nu=0.51, device="cpu").fit(X, y)
    with pytest.raises(ValueError, match="at most 1048576 points"):
        NuSVR(device="cpu").fit(np.zeros((524289, 1)), np.zeros(524289))
