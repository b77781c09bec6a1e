"""Property-based checks of the CPU solvers on random small problems (hypothesis).

The fixed-seed tests pin trajectories bit for bit on MNIST-shaped data; these draw arbitrary shapes,
labels, C and gamma and check what must hold for ANY problem:

* the pairwise SMO oracle (csrc/core/smo_cpu.cpp) and the decomposition oracle (decomp_cpu.cpp) both end
  on the reference's stop test b_low <= b_high + 2 tau (or report why not), inside the box [0, C] with
  sum(alpha y) = 0, and reach the same dual objective;
* the decomposition oracle's distributed form over thread ranks is bit-identical to one rank whenever the
  world divides 8, whatever the working-set size;
* the row-streaming and full-Gram forms of the pairwise oracle agree bit for bit."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from svm355 import SVMParams
from svm355.ops import cpu as C

SETTINGS = settings(max_examples=25, deadline=None, database=None, suppress_health_check=[HealthCheck.too_slow])


def _problem(seed, n, d, pos_frac):
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    y = np.where(rng.random(n) < pos_frac, 1, -1).astype(np.int32)
    y[0], y[1] = 1, -1  # both classes present
    return X, y


def _kernel(X, gamma):
    return C.rbf_matrix(X, X, gamma, 2)


def _gap(K, y, a, p):
    f = K @ (a * y) - y
    hi = ((y == 1) & (a < p.C - p.eps)) | ((y == -1) & (a > p.eps))
    lo = ((y == 1) & (a > p.eps)) | ((y == -1) & (a < p.C - p.eps))
    return f[lo].max() - f[hi].min()


def _dual(K, y, a):
    ay = a * y
    return float(a.sum() - 0.5 * ay @ K @ ay)


problems = st.tuples(st.integers(0, 2**31 - 1), st.integers(12, 160), st.integers(1, 12),
                     st.floats(0.15, 0.85), st.sampled_from([0.5, 1.0, 10.0, 100.0]),
                     st.sampled_from([0.05, 0.5, 2.0, 8.0]))


@SETTINGS
@given(problems, st.sampled_from([16, 64, 1024]))
def test_both_oracles_meet_the_stop_test_at_the_same_optimum(prob, q):
    seed, n, d, pos, Cb, gamma = prob
    X, y = _problem(seed, n, d, pos)
    K = _kernel(X, gamma)
    p = SVMParams(C=Cb, gamma=gamma, n_threads=2, max_iter=200000)
    a1, r1, _ = C.smo_train_gram(K, y, p)
    a2, r2, _, _ = C.decomp_train_gram(K, y, p, q=q)
    for a, r in ((a1, r1), (a2, r2)):
        # a hard draw (large C, tiny gamma) may end on the iteration cap: a reported reason, never silent
        assert r.stop_reason in ("converged", "max_iter", "nonpositive_eta", "infeasible"), r.stop_reason
        # the decomposition oracle floors eta at eps: the reference's eta stop is the pairwise oracle's alone
        assert r is r1 or r.stop_reason != "nonpositive_eta"
        assert np.all((a >= -1e-9) & (a <= Cb + 1e-9))
        assert abs(float(a @ y)) <= 1e-9 * max(1.0, float(a.sum()))
    if r1.stop_reason == r2.stop_reason == "converged":
        assert _gap(K, y, a1, p) <= 2 * p.tau + 1e-9
        assert _gap(K, y, a2, p) <= 2 * p.tau + 1e-9
        w1, w2 = _dual(K, y, a1), _dual(K, y, a2)
        # both are within the stop tolerance of the optimum (over 450 draws the worst relative gap of
        # the dual objectives was 9e-7)
        assert abs(w1 - w2) <= 1e-5 * max(1.0, abs(w1))


@SETTINGS
@given(problems, st.sampled_from([2, 4, 8]), st.sampled_from([64, 1024]))
def test_distributed_decomposition_oracle_is_bit_identical_to_one_rank(prob, world, q):
    seed, n, d, pos, Cb, gamma = prob
    X, y = _problem(seed, n, d, pos)
    K = _kernel(X, gamma)
    p = SVMParams(C=Cb, gamma=gamma, n_threads=1, max_iter=200000)
    a1, r1, s1 = C.decomp_train_gram_dist(K, y, p, world=1, q=q)
    aw, rw, sw = C.decomp_train_gram_dist(K, y, p, world=world, q=q)
    np.testing.assert_array_equal(a1, aw)
    assert (r1.b, r1.iterations, r1.stop_reason) == (rw.b, rw.iterations, rw.stop_reason)
    assert s1["outer_iterations"] == sw["outer_iterations"]


@SETTINGS
@given(problems)
def test_pairwise_oracle_row_and_gram_forms_agree(prob):
    seed, n, d, pos, Cb, gamma = prob
    X, y = _problem(seed, n, d, pos)
    p = SVMParams(C=Cb, gamma=gamma, n_threads=2, max_iter=200000)
    ag, rg, _ = C.smo_train_gram(_kernel(X, gamma), y, p)
    ar, rr = C.smo_train(X, y, p)[:2]
    np.testing.assert_array_equal(ag, ar)
    assert (rg.b, rg.iterations) == (rr.b, rr.iterations)


@pytest.mark.parametrize("n", [3, 5])
def test_tiny_problems(n):
    """Two or three points per class at most: both oracles still end on the stop test."""
    X, y = _problem(7, n, 2, 0.5)
    K = _kernel(X, 1.0)
    p = SVMParams(C=1.0, gamma=1.0, n_threads=1)
    a1, r1, _ = C.smo_train_gram(K, y, p)
    a2, r2, _, _ = C.decomp_train_gram(K, y, p, q=64)
    assert r1.stop_reason == r2.stop_reason == "converged"
    assert _gap(K, y, a1, p) <= 2 * p.tau + 1e-9 and _gap(K, y, a2, p) <= 2 * p.tau + 1e-9
