"""epsilon-SVR on the CPU: the pairwise oracle (``SVR(device="cpu")``, svm_smo_train_svr) and the decomposition
oracle's twin mode (svm_decomp_train_gram_svr) against scikit-learn's fixture, an independent KKT check, the
twin-pair properties over many seeds, the moved-column fold, the edge cases and the refusals."""
import ctypes

import numpy as np
import pytest

from svm355 import SVC, SVR, SVMParams
from svm355 import _native as N
from svm355.models.svr import split_twins
from svm355.ops import cpu as C

from svr_checks import FIXTURE_PRED_TOL, check_kkt, load_fixture, rbf_numpy, real_rows


def _decomp_oracle(X, z, p, epsilon, **kw):
    K = rbf_numpy(X, X, p.gamma)
    a2, res, st, tr = C.decomp_train_gram_svr(K, z, p, epsilon=epsilon, **kw)
    return K, a2, res, st, tr


# ---- scikit-learn fixture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("oracle", ["pairwise", "decomp"])
@pytest.mark.parametrize("seed", [11, 12])
def test_oracles_agree_with_the_scikit_learn_fixture(seed, oracle):
    g = load_fixture(seed)
    X, z, n = g["X"], g["z"], len(g["z"])
    p = SVMParams(C=g["C"], gamma=g["gamma"], tau=1e-6, max_iter=10**7)
    if oracle == "pairwise":
        m = SVR(C=g["C"], gamma=g["gamma"], epsilon=g["epsilon"], tol=1e-6, max_iter=10**7, device="cpu").fit(X, z)
        assert m.stop_reason_ == "converged"
        np.testing.assert_array_equal(m.scaler_.transform(X), X)  # the fixture's rows: scaling is the identity
        pred, beta = m.predict(X), m.alpha_ - m.alpha_star_
    else:
        K, a2, res, _, _ = _decomp_oracle(X, z, p, g["epsilon"])
        assert res.stop_reason == "converged"
        a, a_star = split_twins(a2, p.C)
        beta = a - a_star
        pred = K @ beta - res.b
    err = np.abs(pred - g["pred"]).max()
    print(f"seed {seed} {oracle}: max |prediction - fixture| = {err:.3e} (bound {FIXTURE_PRED_TOL:.1e})")
    assert err <= FIXTURE_PRED_TOL
    # the support may differ only where a coefficient is within 1e-6 of 0 (or of C)
    ours, theirs = np.abs(beta) > p.sv_tol, g["beta"] != 0.0
    for k in np.flatnonzero(ours != theirs):
        v = max(abs(beta[k]), abs(g["beta"][k]))
        assert v <= 1e-6 or v >= p.C - 1e-6, (k, beta[k], g["beta"][k])
    assert abs(int(ours.sum()) - g["n_sv"]) <= int((ours != theirs).sum())


# ---- independent KKT check --------------------------------------------------------------------------------------
@pytest.mark.parametrize("oracle", ["pairwise", "decomp"])
@pytest.mark.parametrize("epsilon", [0.1, 0.0])
def test_kkt_from_an_independent_rbf(oracle, epsilon):
    X, z = real_rows(250, seed=21)
    p = SVMParams(C=10.0, gamma=0.5, tau=1e-5, max_iter=10**7)
    K = rbf_numpy(X, X, p.gamma)
    if oracle == "pairwise":
        a2, res = C.smo_train_svr(X, z, p, epsilon)
    else:
        a2, res, _, _ = C.decomp_train_gram_svr(K, z, p, epsilon=epsilon, q=256)
    assert res.stop_reason == "converged"
    a, a_star = split_twins(a2, p.C)
    assert np.abs(a2 - np.concatenate([a, a_star])).max() <= 1e-14  # what the clamp removes: a few ulp of C
    check_kkt(K, z, a, a_star, res.b, C=p.C, epsilon=epsilon, tau=p.tau)


# ---- the twin pair over many seeds ------------------------------------------------------------------------------
# A twin pair has eta = 0, and the reference stops at eta <= eps (SVM_STOP_NONPOS_ETA).  (high = k, low = k + n) is
# never violating, f_{k+n} = f_k - 2 epsilon; (high = k + n, low = k) needs a_k and a*_k inside the box at once.
# Measured on these shapes (the decomposition oracle, 20 seeds at n = 50 / 300, 2 at 1,537):
#   epsilon = 0.3   a_k a*_k = 0 exactly after every outer iteration, on every shape;
#   epsilon = 0.05  in 3-13 of 20 solves per shape a variable the pair update brought back to 0 keeps a residue of
#                   at most 6.7e-16 (the update moves the unclipped variable by the clipped one's change, so it
#                   lands within a few ulp of the bound, not on it) while its twin grows: the product is ~1e-15,
#                   not 0.  Such a value is at the bound for every set-membership test (a > eps = 1e-12), so the
#                   degenerate pair cannot be selected; the property asserted is min(a_k, a*_k) <= eps;
#   epsilon = 0     dropped from the product property: the twins' f are equal and the objective is flat along
#                   a_k = a*_k, so both grow together (min(a_k, a*_k) up to 9.1 at C = 10); only beta is
#                   determined.  The twin pair is still never violating (f_k = f_{k+n}), and the solve must end
#                   converged like every other.
# No solve ended in SVM_STOP_NONPOS_ETA, and every solve converged.
# (Identical ROWS with different targets are the other source of eta = 0: test_decomp_degenerate_cpu.py.)
_SEEDS = {50: 20, 300: 20, 1537: 2}


@pytest.mark.parametrize("q", [64, 256])
@pytest.mark.parametrize("epsilon", [0.0, 0.05, 0.3])
@pytest.mark.parametrize("n", [50, 300, 1537])
def test_twins_never_both_inside_the_box(n, epsilon, q):
    seeds = _SEEDS[n] if epsilon > 0 else max(1, _SEEDS[n] // 10)  # epsilon = 0: convergence only, long solves
    p = SVMParams(C=10.0, gamma=0.5, tau=1e-5, max_iter=10**7, n_threads=4)
    for seed in range(seeds):
        X, z = real_rows(n, seed=seed * 7 + n)
        K = rbf_numpy(X, X, p.gamma)
        if epsilon == 0.0:
            _, res, _, _ = C.decomp_train_gram_svr(K, z, p, epsilon=epsilon, q=q)
            assert res.stop_reason == "converged", (seed, res.stop_reason)
            continue
        _, _, st, _ = C.decomp_train_gram_svr(K, z, p, epsilon=epsilon, q=q)
        _, res, st2, tr = C.decomp_train_gram_svr(K, z, p, epsilon=epsilon, q=q, trace_cap=st["outer_iterations"] + 1,
                                                  snapshots=True)
        assert res.stop_reason == "converged", (seed, res.stop_reason)
        assert tr.count == st2["outer_iterations"] == st["outer_iterations"] > 0
        al = tr.alpha[: tr.count]
        both = np.minimum(al[:, :n], al[:, n:])
        assert both.max() <= p.eps, (seed, both.max())
        if epsilon == 0.3:
            assert not (al[:, :n] * al[:, n:]).any(), seed


def test_pairwise_oracle_keeps_the_twins_apart():
    for seed in range(20):
        X, z = real_rows(120, seed=seed)
        a2, res = C.smo_train_svr(X, z, SVMParams(C=10.0, gamma=0.5, max_iter=10**7), 0.05)
        assert res.stop_reason == "converged"
        assert np.minimum(a2[:120], a2[120:]).max() <= 1e-12


# ---- the moved-column fold --------------------------------------------------------------------------------------
def test_fold_positions_coefficients_and_count():
    n = 100
    #       k then k+n   k+n then k    lone a   lone a*   k then k+n again (far apart)
    cols = [7, 107, 150, 50, 3, 199, 20, 64, 120]
    coef = [1.5, -0.25, 2.0, 0.125, -3.0, 4.0, 1e-3, 0.5, 1e13]
    rows, rc = C.twin_fold(np.array(cols), np.array(coef), n)
    np.testing.assert_array_equal(rows, [7, 50, 3, 99, 20, 64])  # first occurrences, in list order
    # coef_k + coef_{k+n}, in that order, whichever came first in the list
    np.testing.assert_array_equal(rc, [1.5 + -0.25, 0.125 + 2.0, -3.0, 4.0, 1e-3 + 1e13, 0.5])
    rows, rc = C.twin_fold(np.array([], dtype=np.int32), np.array([]), n)
    assert rows.size == 0 and rc.size == 0
    with pytest.raises(N.NativeError, match="outside"):
        C.twin_fold(np.array([200]), np.array([1.0]), n)


# ---- edges ------------------------------------------------------------------------------------------------------
def test_tube_wider_than_the_targets_spread():
    """2 epsilon >= max z - min z: the start already meets the stop test (b_high = epsilon - max z, b_low =
    -epsilon - min z), so no update runs, no support vector exists and the prediction is the mid-range."""
    X, z = real_rows(80, seed=4)
    eps = (z.max() - z.min()) / 2
    m = SVR(epsilon=eps, gamma=0.5, device="cpu").fit(X, z)
    assert m.stop_reason_ == "converged" and m.n_iter_ == 1  # the solvers' count is updates + 1
    assert len(m.support_) == 0 and m.dual_coef_.size == 0
    np.testing.assert_array_equal(m.predict(X[:7]), np.full(7, (z.max() + z.min()) / 2))
    K, a2, res, st, _ = _decomp_oracle(X, z, SVMParams(gamma=0.5), eps)
    assert st["outer_iterations"] == 0 and res.iterations == 1 and not a2.any()
    assert res.b == -(z.max() + z.min()) / 2


def test_constant_target_and_two_rows():
    X, _ = real_rows(40, seed=8)
    m = SVR(epsilon=0.0, gamma=0.5, device="cpu").fit(X, np.full(40, 1.25))
    assert len(m.support_) == 0 and m.n_iter_ == 1
    np.testing.assert_array_equal(m.predict(X[:3]), 1.25)
    X2, z2 = np.array([[0.0, 1.0], [1.0, 0.0]]), np.array([-1.0, 2.0])
    for eps in (0.0, 0.1):
        m = SVR(C=10.0, gamma=0.5, epsilon=eps, device="cpu").fit(X2, z2)
        assert m.stop_reason_ == "converged"
        # two rows: beta = (-t, t), pred_k = z_k -+ epsilon when t < C (a free pair sits on the tube's edge)
        t = m.alpha_[1] - m.alpha_star_[1]
        assert 0 < t < 10.0 and abs(m.alpha_star_[0] - t) < 1e-12
        assert np.abs(m.predict(X2) - (z2 + [eps, -eps])).max() <= 1e-5 + 1e-9
        K = rbf_numpy(X2, X2, 0.5)
        a2, res, _, _ = C.decomp_train_gram_svr(K, z2, SVMParams(gamma=0.5), epsilon=eps)
        assert res.stop_reason == "converged" and abs((a2[1] - a2[3]) - t) <= 1e-4


def test_epsilon_zero_interpolates_within_the_stop_tolerance():
    X, z = real_rows(60, seed=3, noise=0.0)
    m = SVR(C=1e4, gamma=2.0, epsilon=0.0, device="cpu", max_iter=10**7).fit(X, z)
    assert m.stop_reason_ == "converged"
    assert np.abs(m.predict(X) - z).max() <= m.params.tau + 1e-9  # every variable is free: |r| <= tau
    assert m.score(X, z) > 1 - 1e-8


# ---- refusals ---------------------------------------------------------------------------------------------------
def test_fit_refuses_bad_arguments():
    X, z = real_rows(30, seed=1)
    with pytest.raises(ValueError, match="epsilon"):
        SVR(epsilon=-0.1)
    with pytest.raises(ValueError, match="epsilon"):
        SVR(epsilon=float("nan"))
    with pytest.raises(ValueError, match="C"):
        SVR(C=0.0)
    for bad in (np.nan, np.inf):
        zz = z.copy()
        zz[3] = bad
        with pytest.raises(ValueError, match="NaN or infinite"):
            SVR(device="cpu").fit(X, zz)
    with pytest.raises(ValueError, match="z"):
        SVR(device="cpu").fit(X, z[:-1])
    with pytest.raises(ValueError, match="scale=True"):  # before any device work: no GPU is needed to refuse
        SVR(device="cuda", scale=False).fit(X, z)


def test_oracles_refuse_what_twin_mode_does_not_cover(monkeypatch):
    X, z = real_rows(30, seed=1)
    K = rbf_numpy(X, X, 0.5)
    for p, what in ((SVMParams(shrinking=True), "shrinking"), (SVMParams(weight_pos=2.0), "class weights"),
                    (SVMParams(weight_neg=0.5), "class weights")):
        with pytest.raises(N.NativeError, match=what):
            C.decomp_train_gram_svr(K, z, p)
    with pytest.raises(N.NativeError, match="class weights"):
        C.smo_train_svr(X, z, SVMParams(weight_pos=2.0))
    with pytest.raises(N.NativeError, match="epsilon"):
        C.decomp_train_gram_svr(K, z, SVMParams(), epsilon=-1.0)
    zz = z.copy()
    zz[5] = np.inf
    with pytest.raises(N.NativeError, match="not finite"):
        C.decomp_train_gram_svr(K, zz, SVMParams())
    monkeypatch.setenv("SVM355_DECOMP_NEWTON", "1")
    with pytest.raises(N.NativeError, match="Newton"):
        C.decomp_train_gram_svr(K, z, SVMParams())
    monkeypatch.delenv("SVM355_DECOMP_NEWTON")
    # 2 n > 2^31 - 1 points: refused from the sizes alone, before K or z is read
    big = 2**30
    a = np.zeros(4)
    r, p = N.SvmResult(), SVMParams().to_struct()
    rc = N.core().svm_decomp_train_gram_svr(N.ptr(K), big, N.ptr(z), big, 0.1, N.ptr(a), ctypes.byref(p), 1024, 0.1, 3,
                                            0, ctypes.byref(r), None, None)
    assert rc == 2 and "2^31 - 1" in N.last_error()


# ---- persistence ------------------------------------------------------------------------------------------------
def test_save_load_round_trip_and_kinds(tmp_path):
    X, z = real_rows(150, seed=6)
    Xq, _ = real_rows(40, seed=7, bounds_of=X)
    m = SVR(C=5.0, gamma=0.5, epsilon=0.07, device="cpu").fit(X, z)
    assert 0 < len(m.support_) < 150 and (m.dual_coef_ < 0).any() and (m.dual_coef_ > 0).any()
    m.save(tmp_path / "svr")
    back = SVR.load(tmp_path / "svr")
    np.testing.assert_array_equal(back.predict(Xq), m.predict(Xq))
    np.testing.assert_array_equal(back.support_, m.support_)
    np.testing.assert_array_equal(back.dual_coef_, m.dual_coef_)
    assert back.epsilon == 0.07 and back.params.C == 5.0 and back.b_ == m.b_ and back.intercept_ == -m.b_
    with pytest.raises(ValueError, match="not a classifier"):
        SVC.load(tmp_path / "svr")
    c = SVC(device="cpu", gamma=0.5).fit(X, np.where(z > np.median(z), 1, -1).astype(np.int32))
    c.save(tmp_path / "svc")
    with pytest.raises(ValueError, match="not an SVR"):
        SVR.load(tmp_path / "svc")
    assert np.array_equal(SVC.load(tmp_path / "svc").predict(Xq), c.predict(Xq))


def test_fit_attributes():
    X, z = real_rows(100, seed=12)
    m = SVR(C=10.0, gamma=0.5, epsilon=0.1, device="cpu").fit(X, z)
    beta = m.alpha_ - m.alpha_star_
    np.testing.assert_array_equal(m.support_, np.flatnonzero(np.abs(beta) > m.params.sv_tol))
    np.testing.assert_array_equal(m.dual_coef_, beta[m.support_])
    assert m.intercept_ == -m.b_ and m.n_iter_ > 1 and m.stop_reason_ == "converged" and "smo_ms" in m.timings_
    pred = rbf_numpy(X, X, 0.5) @ beta - m.b_
    assert np.abs(m.predict(X) - pred).max() < 1e-12
    assert abs(m.score(X, z) - (1 - ((z - pred) ** 2).sum() / ((z - z.mean()) ** 2).sum())) < 1e-12
