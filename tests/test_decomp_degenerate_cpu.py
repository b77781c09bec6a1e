"""The decomposition oracle (csrc/core/decomp_cpu.cpp) on training sets with identical rows that carry
conflicting labels or different targets (degenerate_checks.py has the cases).

Two such rows have K = 1 and eta = 0, and their pair is violating until one of them sits at its bound.  The
second-order choice of j prefers exactly that pair (its gain is -(f_j - f_i)^2 / eps), so every inner_wss >= 2
meets it; the update floors eta at eps and the box clips the step.  Checked here, on the CPU:

* every case converges for inner_wss 1 / 2 / 3 / 4 and q = 64 / 1024 and ends on the reference's stop test,
  recomputed from an independent numpy FP64 RBF (direct squared differences); the regression cases meet the
  KKT conditions of svr_checks.check_kkt;
* every conflicting pair of a classifier ends with at least one member at C;
* the oracle's eta_floor_updates counter shows that the floored update ran (inner_wss >= 2; the first-order
  choice of inner_wss 1 takes the largest f, not the copy, and is only required to converge);
* scikit-learn's solutions of two such problems (tests/golden/degenerate_*.npz);
* a hypothesis property over heavily duplicated low-range integer data, which floors on every draw."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings

from svm355 import SVMParams
from svm355.models.svr import split_twins
from svm355.ops import cpu as C

import degenerate_checks as G
from svr_checks import check_kkt

SETTINGS = settings(max_examples=25, deadline=None, database=None, suppress_health_check=[HealthCheck.too_slow])
ARMS = [(q, w) for q in G.WORKING_SETS for w in G.INNER_WSS]


def _kernels(X, gamma):
    """(the oracle's kernel matrix: the library's reference RBF with a unit diagonal; the independent one)."""
    Xs = G.scaled(X)
    K = C.rbf_matrix(Xs, Xs, gamma, 4)
    np.fill_diagonal(K, 1.0)
    Ki = G.rbf_direct(Xs, gamma)
    for A in (K, Ki):
        A.flags.writeable = False
    return K, Ki


def _classifier_checks(K, Ki, y, pairs, p, q, wss):
    a, r, st, _ = C.decomp_train_gram(K, y, p, q=q, inner_wss=wss)
    print(f"q={q} inner_wss={wss}: {r.stop_reason} after {r.iterations} iterations, "
          f"{st['eta_floor_updates']} floored updates, gap {G.gap(Ki, y, a, p.C):.3e}")
    assert r.stop_reason == "converged"
    assert G.gap(Ki, y, a, p.C) <= 2 * p.tau + 1e-9
    assert G.pairs_rest_at_a_bound(a, pairs, p.C)
    assert np.all((a >= -1e-9) & (a <= p.C + 1e-9)) and abs(float(a @ y)) <= 1e-9 * max(1.0, a.sum())
    if wss >= 2:
        assert st["eta_floor_updates"] > 0, "the inputs no longer reach the floored update"
    return a, r


# ---- (a) pixel classifier ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=G.PIXEL_SIZES, ids=lambda s: f"{s[0]}+{s[1]}")
def pixel_case(request):
    X, y, pairs = G.pixel_classifier(*request.param)
    K, Ki = _kernels(X, G.PIXEL_GAMMA)
    assert np.all(K[pairs[:, 0], pairs[:, 1]] == 1.0) and np.all(Ki[pairs[:, 0], pairs[:, 1]] == 1.0)
    return K, Ki, y, pairs


@pytest.mark.parametrize("q,wss", ARMS)
def test_pixel_classifier_with_conflicting_copies(pixel_case, q, wss):
    K, Ki, y, pairs = pixel_case
    _classifier_checks(K, Ki, y, pairs, SVMParams(n_threads=4), q, wss)


# ---- (b) real-valued classifier ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_case():
    X, y, pairs = G.real_classifier()
    return (*_kernels(X, G.REAL_GAMMA), y, pairs)


@pytest.mark.parametrize("q,wss", ARMS)
def test_real_valued_classifier_with_conflicting_copies(real_case, q, wss):
    K, Ki, y, pairs = real_case
    _classifier_checks(K, Ki, y, pairs, SVMParams(C=10.0, gamma=G.REAL_GAMMA, n_threads=4, max_iter=10**7), q, wss)


def test_a_curvature_between_zero_and_eps_is_floored_too():
    """FP64-MFMA kernel values between two copies are 1 or 1 - ulp: eta = 2.2e-16 <= eps.  The same solve with
    those entries one ulp below 1 still converges, floors, and ends within the stop tolerance of the same b."""
    X, y, pairs = G.real_classifier()
    K, Ki = _kernels(X, G.REAL_GAMMA)
    Ku = K.copy()
    i, j = pairs[::2, 0], pairs[::2, 1]  # every other pair: both eta = 0 and 0 < eta <= eps occur
    Ku[i, j] = Ku[j, i] = np.nextafter(1.0, 0.0)
    p = SVMParams(C=10.0, gamma=G.REAL_GAMMA, n_threads=4, max_iter=10**7)
    a, r, st, _ = C.decomp_train_gram(Ku, y, p)
    ref, rr, _, _ = C.decomp_train_gram(K, y, p)
    assert r.stop_reason == rr.stop_reason == "converged" and st["eta_floor_updates"] > 0
    assert G.gap(Ki, y, a, p.C) <= 2 * p.tau + 1e-9
    assert G.pairs_rest_at_a_bound(a, pairs, p.C) and abs(r.b - rr.b) <= 10 * p.tau


# ---- (c) regression: replicated rows with different targets -----------------------------------------------------
@pytest.fixture(scope="module", params=["real", "pixel"])
def svr_case(request):
    X, z = G.real_svr() if request.param == "real" else G.pixel_svr()
    gamma = G.REAL_GAMMA if request.param == "real" else G.PIXEL_GAMMA
    return (*_kernels(X, gamma), z, gamma, (0.1 if request.param == "real" else 0.05))


@pytest.mark.parametrize("q,wss", ARMS)
@pytest.mark.parametrize("tube", ["epsilon", "zero"])
def test_svr_with_replicated_rows(svr_case, tube, q, wss):
    """epsilon = 0.1 (real rows) / 0.05 (pixel rows), and epsilon = 0, where replicates whose targets differ by
    more than 2 tau are violating (every replicate's target here differs by far more)."""
    K, Ki, z, gamma, epsilon = svr_case
    epsilon = epsilon if tube == "epsilon" else 0.0
    p = SVMParams(C=10.0, gamma=gamma, n_threads=4, max_iter=10**7)
    a2, r, st, _ = C.decomp_train_gram_svr(K, z, p, epsilon=epsilon, q=q, inner_wss=wss)
    print(f"epsilon={epsilon} q={q} inner_wss={wss}: {r.stop_reason} after {r.iterations} iterations, "
          f"{st['eta_floor_updates']} floored updates")
    assert r.stop_reason == "converged"
    a, a_star = split_twins(a2, p.C)
    check_kkt(Ki, z, a, a_star, r.b, C=p.C, epsilon=epsilon, tau=p.tau)
    if wss >= 2:
        assert st["eta_floor_updates"] > 0, "the inputs no longer reach the floored update"


# ---- scikit-learn fixtures --------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,wss", ARMS)
def test_svr_fixture_predictions(q, wss):
    g = G.load_fixture("svr_n240")
    X, z = G.real_svr()
    np.testing.assert_array_equal(g["X"], X)  # the fixture's rows are the case's
    np.testing.assert_array_equal(g["z"], z)
    K = G.rbf_direct(X, g["gamma"])
    p = SVMParams(C=g["C"], gamma=g["gamma"], tau=1e-6, max_iter=10**7, n_threads=4)
    a2, r, st, _ = C.decomp_train_gram_svr(K, z, p, epsilon=g["epsilon"], q=q, inner_wss=wss)
    assert r.stop_reason == "converged"
    a, a_star = split_twins(a2, p.C)
    err = np.abs(K @ (a - a_star) - r.b - g["pred"]).max()
    print(f"q={q} inner_wss={wss}: max |prediction - fixture| = {err:.3e} (bound {G.FIXTURE_SVR_TOL:.1e})")
    assert err <= G.FIXTURE_SVR_TOL
    if wss >= 2:
        assert st["eta_floor_updates"] > 0


@pytest.mark.parametrize("q,wss", ARMS)
def test_svc_fixture_decision_values(q, wss):
    g = G.load_fixture("svc_n330")
    X, y, pairs = G.svc_fixture_rows()
    np.testing.assert_array_equal(g["X"], X)
    np.testing.assert_array_equal(g["y"], y)
    K = G.rbf_direct(G.scaled(X), g["gamma"])
    p = SVMParams(C=g["C"], gamma=g["gamma"], tau=1e-6, max_iter=10**7, n_threads=4)
    a, r, st, _ = C.decomp_train_gram(K, y, p, q=q, inner_wss=wss)
    assert r.stop_reason == "converged"
    err = np.abs(K @ (a * y) - r.b - g["dec"]).max()
    print(f"q={q} inner_wss={wss}: max |decision - fixture| = {err:.3e} (bound {G.FIXTURE_SVC_TOL:.1e})")
    assert err <= G.FIXTURE_SVC_TOL
    assert G.pairs_rest_at_a_bound(a, pairs, p.C)
    if wss >= 2:
        assert st["eta_floor_updates"] > 0


# ---- (d) heavily duplicated low-range integer data --------------------------------------------------------------
@SETTINGS
@given(G.low_range_strategy())
def test_low_range_integer_data_ends_on_the_stop_test(prob):
    """4 - 256 distinct rows for 200 - 1500 points, random labels and targets: most rows have copies of both
    classes.  The oracle reports converged or max_iter (never the reference's eta stop), both solves floor, and
    a converged solve meets the stop test / the KKT conditions from the independent kernel."""
    seed, n, d, vmax, Cb, gamma = prob
    X, y, z = G.low_range_problem(seed, n, d, vmax)
    K, Ki = _kernels(X, gamma)
    p = SVMParams(C=Cb, gamma=gamma, n_threads=4)
    a, r, st, _ = C.decomp_train_gram(K, y, p)
    assert r.stop_reason in ("converged", "max_iter"), r.stop_reason
    assert st["eta_floor_updates"] > 0, "the inputs no longer reach the floored update"
    assert np.all((a >= -1e-9) & (a <= Cb + 1e-9)) and abs(float(a @ y)) <= 1e-9 * max(1.0, a.sum())
    if r.stop_reason == "converged":
        assert G.gap(Ki, y, a, Cb) <= 2 * p.tau + 1e-9
    a2, r2, st2, _ = C.decomp_train_gram_svr(K, z, p, epsilon=0.1)
    assert r2.stop_reason in ("converged", "max_iter"), r2.stop_reason
    assert st2["eta_floor_updates"] > 0, "the inputs no longer reach the floored update"
    if r2.stop_reason == "converged":
        aa, a_star = split_twins(a2, Cb)
        check_kkt(Ki, z, aa, a_star, r2.b, C=Cb, epsilon=0.1, tau=p.tau)
