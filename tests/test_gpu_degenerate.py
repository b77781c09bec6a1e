"""Identical rows with conflicting labels (or different targets) on the device decomposition solver
(ws_inner_kernel, csrc/hip/decomp_inner.hip) against its CPU oracle, the pairwise device solver against the
pairwise oracle, and both against references of their own (degenerate_checks.py has the cases).

Two copies of a row have K = 1 (exact-integer path) or 1 / 1 - ulp (FP64-MFMA values), so their pair has
eta <= eps and is violating until one of them sits at its bound.  The decomposition solver floors eta at eps and
lets the box clip the step; the pairwise solvers keep the reference's stop (SVM_STOP_NONPOS_ETA).

* The whole solve bit for bit against the oracle run on the device's own kernel values: every outer iteration's
  working set, inner count, bounds, moved list, coefficients, alpha and f, the final alpha, b, iterations and
  "converged" -- with the copies inside one working set and spread over many, on uint8 and FP64 rows, for the
  classifier and the regression (twin) solve.  The oracle's eta_floor_updates > 0 shows that the inputs reach
  the floored update (the device does not count; its trace is the oracle's).
* The inner kernel's arms on a problem of fewer points than the working set holds (every selection is the whole
  problem: a step-level test of ws_inner_kernel): the selection rules, the workgroup shapes, the weighted kernel,
  the Newton variant, the column cache, shrinking.
* The stop test on all points from an independent FP64 kernel, every conflicting pair with a member at its bound,
  scikit-learn's fixtures, the estimators with default arguments, the two-rank rehearsal, the pairwise solver.
"""
import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings

from svm355 import SVC, SVR, OneVsRestSVC, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C
from svm355.ops import device as D
from svm355.utils.data import synthetic_mnist

import degenerate_checks as G
from decomp_checks import kkt_gap_fp64
from svr_checks import check_kkt

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SETTINGS = settings(max_examples=20, deadline=None, database=None,
                    suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture])
AGGRESSIVE = {"SVM355_DECOMP_SHRINK": "1", "SVM355_DECOMP_SHRINK_START": "1", "SVM355_DECOMP_SHRINK_MARGIN": "0"}
NEWTON = {"SVM355_DECOMP_NEWTON": "1", "SVM355_DECOMP_NEWTON_EVERY": "5", "SVM355_DECOMP_NEWTON_FRAC": "0"}


# ---- rows on the device and the device's own kernel values on the host ------------------------------------------
def _u8_problem(X, gamma):
    """uint8 rows: (device rows, column min, column max, the exact-integer Gram on the host)."""
    n, d = X.shape
    Xu = D.upload_u8(np.ascontiguousarray(X), DEV)
    mmd = torch.empty(2 * d, dtype=torch.float64, device=DEV)
    D.minmax_u8(Xu, out=mmd)
    mm = mmd.cpu().numpy()
    mn, mx = mm[:d].copy(), mm[d:].copy()
    Kd = D.rbf_gram_u8(Xu, gamma, mn, mx)
    assert Kd is not None, "no exact-integer plan for these integer rows"
    K = np.ascontiguousarray(Kd[:n, :n].cpu().numpy())
    del Kd
    D.release_gram_buffers()
    torch.cuda.empty_cache()
    return Xu, mn, mx, K


def _f64_problem(X, gamma):
    """Real-valued rows (min-max scaling is the identity on them): the solve's own FP64-MFMA kernel values."""
    n, d = X.shape
    Xd = D.upload_rows(np.ascontiguousarray(X), DEV)
    mn, mx, _ = D.minmax_scale_(Xd, d)
    nrm = D.row_norms(Xd, d)
    K = np.ascontiguousarray(D.rbf_gram(Xd, nrm, Xd, nrm, gamma, symmetric=True)[:n, :n].cpu().numpy())
    return Xd, mn.cpu().numpy(), mx.cpu().numpy(), K


def _compare(dt, ot):
    dr, orr = dt.records(), ot.records()
    assert len(dr) == len(orr) and len(dr) > 0
    for o, (a, b) in enumerate(zip(dr, orr)):
        assert a["m"] == b["m"], o
        np.testing.assert_array_equal(a["W"], b["W"], err_msg=f"outer {o}: working set")
        assert a["inner"] == b["inner"], o
        np.testing.assert_array_equal(a["bounds"], b["bounds"], err_msg=f"outer {o}: bounds")
        np.testing.assert_array_equal(a["cols"], b["cols"], err_msg=f"outer {o}: moved points")
        np.testing.assert_array_equal(a["coef"], b["coef"], err_msg=f"outer {o}: coefficients")
        np.testing.assert_array_equal(a["alpha"], b["alpha"], err_msg=f"outer {o}: alpha")
        np.testing.assert_array_equal(a["f"], b["f"], err_msg=f"outer {o}: f")  # NaN = shrunk, on both sides
    return len(dr)


def _classifier_trajectory(Xdev, mn, mx, K, y, p, q=1024, inner_wss=3, fp64_rows=False, cap=400, floors=True):
    n = len(y)
    yd = torch.from_numpy(np.array(y, dtype=np.int32)).to(DEV)
    alpha = torch.empty(n, dtype=torch.float64, device=DEV)
    dt = N.DecompTrace(cap, n)
    out = D.train_decomp(Xdev, yd, alpha, p, mn, mx, working_set=q, trace=dt)
    assert out is not None
    res, tm = out
    a_o, r_o, st_o, ot = C.decomp_train_gram(K, y, p.replace(n_threads=8), q=q, inner_wss=inner_wss, trace_cap=cap,
                                             snapshots=True, fp64_rows=fp64_rows)
    assert st_o["eta_floor_updates"] > 0 or not floors, "the inputs no longer reach the floored update"
    outers = _compare(dt, ot)
    assert res.stop_reason == r_o.stop_reason == "converged"
    assert res.iterations == r_o.iterations and res.b == r_o.b
    a = alpha.cpu().numpy()
    np.testing.assert_array_equal(a, a_o)
    assert tm["outer_iterations"] == st_o["outer_iterations"] == outers and tm["working_set"] == st_o["working_set"]
    return a, tm, st_o


def _svr_trajectory(Xdev, mn, mx, K, z, p, epsilon, q=1024, fp64_rows=False, cap=400):
    n = len(z)
    zd = torch.from_numpy(np.array(z, dtype=np.float64)).to(DEV)
    alpha = torch.empty(2 * n, dtype=torch.float64, device=DEV)
    dt = N.DecompTrace(cap, 2 * n)
    out = D.train_decomp_svr(Xdev, zd, alpha, p, mn, mx, epsilon=epsilon, working_set=q, trace=dt)
    assert out is not None
    res, tm = out
    a_o, r_o, st_o, ot = C.decomp_train_gram_svr(K, z, p.replace(n_threads=8), epsilon=epsilon, q=q, trace_cap=cap,
                                                 snapshots=True, fp64_rows=fp64_rows)
    assert st_o["eta_floor_updates"] > 0, "the inputs no longer reach the floored update"
    outers = _compare(dt, ot)
    assert res.stop_reason == r_o.stop_reason == "converged"
    assert res.iterations == r_o.iterations and res.b == r_o.b
    a2 = alpha.cpu().numpy()
    np.testing.assert_array_equal(a2, a_o)
    assert tm["outer_iterations"] == st_o["outer_iterations"] == outers
    return a2, res, tm


def _torch_rbf(X, gamma):
    """The regression checks' independent kernel: torch cdist on the min-max scaled rows, no matmul."""
    Xt = torch.from_numpy(G.scaled(X)).to(DEV)
    d2 = torch.cdist(Xt, Xt, compute_mode="donot_use_mm_for_euclid_dist") ** 2
    return torch.exp(-gamma * d2).cpu().numpy()


def _weighted_gap_fp64(X, y, a, p):
    """decomp_checks.kkt_gap_fp64 over the per-class boxes."""
    Xs = torch.from_numpy(G.scaled(X)).to(DEV)
    sq = (Xs * Xs).sum(1)
    Kb = torch.exp(-p.gamma * torch.clamp(sq[:, None] + sq[None, :] - 2.0 * (Xs @ Xs.T), min=0.0))
    f = (Kb @ torch.from_numpy(a * y).to(DEV)).cpu().numpy() - y
    box = p.box(y)
    hi = ((y == 1) & (a < box - p.eps)) | ((y == -1) & (a > p.eps))
    lo = ((y == 1) & (a > p.eps)) | ((y == -1) & (a < box - p.eps))
    return f[lo].max() - f[hi].min()


# ---- (a) pixel classifier: the copies inside one working set and spread over many -------------------------------
@pytest.fixture(scope="module", params=G.PIXEL_SIZES, ids=lambda s: f"{s[0]}+{s[1]}")
def pixel_case(request):
    X, y, pairs = G.pixel_classifier(*request.param)
    return (X, y, pairs, *_u8_problem(X, G.PIXEL_GAMMA))


@pytest.mark.parametrize("q", G.WORKING_SETS)
def test_pixel_classifier_trajectory_equals_the_oracle(pixel_case, q):
    X, y, pairs, Xu, mn, mx, K = pixel_case
    assert np.all(K[pairs[:, 0], pairs[:, 1]] == 1.0)  # eta = 0 exactly
    p = SVMParams()
    a, tm, _ = _classifier_trajectory(Xu, mn, mx, K, y, p, q=q)
    assert tm["gram_path"] == "int8-exact"
    assert kkt_gap_fp64(X, y.astype(np.float64), a, p) <= 2 * p.tau + 1e-9
    assert G.pairs_rest_at_a_bound(a, pairs, p.C)


# ---- the inner kernel's arms on fewer points than the working set holds -----------------------------------------
@pytest.fixture(scope="module")
def small_pixel_case():
    X, y, pairs = G.pixel_classifier(*G.PIXEL_SIZES[0])
    assert len(y) <= 1024
    return (X, y, pairs, *_u8_problem(X, G.PIXEL_GAMMA))


@pytest.mark.parametrize("wss", [1, 2, 3, 4])
def test_inner_selection_rules(small_pixel_case, wss, monkeypatch):
    """SVM355_DECOMP_WSS = 1 / 2 / 3 / 4 (oracle inner_wss).  The first-order rule takes the largest f, not the
    copy, and never floors: it is compared all the same (the oracle's counter is 0 there)."""
    monkeypatch.setenv("SVM355_DECOMP_WSS", str(wss))
    X, y, pairs, Xu, mn, mx, K = small_pixel_case
    p = SVMParams()
    a, _, st_o = _classifier_trajectory(Xu, mn, mx, K, y, p, inner_wss=wss, floors=wss >= 2)
    assert wss >= 2 or st_o["eta_floor_updates"] == 0
    assert kkt_gap_fp64(X, y.astype(np.float64), a, p) <= 2 * p.tau + 1e-9
    assert G.pairs_rest_at_a_bound(a, pairs, p.C)


@pytest.mark.parametrize("env", [{"SVM355_DECOMP_NT": "64"}, {"SVM355_DECOMP_NT": "128"}, {"SVM355_DECOMP_NT": "512"},
                                 {"SVM355_DECOMP_CCACHE": "1"}, AGGRESSIVE, NEWTON, {**NEWTON, "SVM355_DECOMP_NT": "64"}],
                         ids=lambda e: "-".join(f"{k[14:]}{v}" for k, v in e.items()))
def test_inner_kernel_arms(small_pixel_case, env, monkeypatch):
    """The workgroup shapes (the oracle reads SVM355_DECOMP_NT too: the second pair's i2 depends on it), the
    column cache forced on, shrinking under LIBSVM's rule every outer iteration, the Newton variant."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    X, y, pairs, Xu, mn, mx, K = small_pixel_case
    p = SVMParams()
    a, tm, st_o = _classifier_trajectory(Xu, mn, mx, K, y, p)
    if "SVM355_DECOMP_NT" in env:
        assert tm["inner_threads"] == int(env["SVM355_DECOMP_NT"])
    if "SVM355_DECOMP_SHRINK" in env:
        assert tm["shrink_passes"] == st_o["shrink_passes"] >= 1 and tm["unshrinks"] == st_o["unshrinks"]
    if "SVM355_DECOMP_NEWTON" in env:
        assert tm["newton_steps"] == st_o["newton_steps"]
    assert kkt_gap_fp64(X, y.astype(np.float64), a, p) <= 2 * p.tau + 1e-9
    assert G.pairs_rest_at_a_bound(a, pairs, p.C)


def test_weighted_inner_kernel(small_pixel_case):
    X, y, pairs, Xu, mn, mx, K = small_pixel_case
    p = SVMParams(weight_pos=2.0, weight_neg=0.5)
    a, _, _ = _classifier_trajectory(Xu, mn, mx, K, y, p)
    assert _weighted_gap_fp64(X, y.astype(np.float64), a, p) <= 2 * p.tau + 1e-9
    box = p.box(y)
    i, j = pairs[:, 0], pairs[:, 1]
    assert np.all((a[i] >= box[i] - p.eps) | (a[j] >= box[j] - p.eps))
    assert a.max() > p.C


# ---- (b) real-valued classifier: FP64-MFMA kernel values --------------------------------------------------------
@pytest.mark.parametrize("q", G.WORKING_SETS)
def test_real_valued_classifier_trajectory_equals_the_oracle(q):
    X, y, pairs = G.real_classifier()
    p = SVMParams(C=10.0, gamma=G.REAL_GAMMA)
    Xd, mn, mx, K = _f64_problem(X, p.gamma)
    kc = K[pairs[:, 0], pairs[:, 1]]
    print(f"K between copies: {np.count_nonzero(kc == 1.0)} x 1, {np.count_nonzero(kc != 1.0)} x other, "
          f"min {kc.min()!r}")
    assert np.all(2.0 - 2.0 * kc <= p.eps)  # eta = 0 or a few ulp: floored either way
    assert np.any(kc == 1.0) and np.any(kc != 1.0)  # both eta = 0 and 0 < eta <= eps are among the pairs
    a, tm, _ = _classifier_trajectory(Xd, mn, mx, K, y, p, q=q, fp64_rows=True, cap=700)
    assert tm["gram_path"] == "fp64"
    assert kkt_gap_fp64(X, y.astype(np.float64), a, p) <= 2 * p.tau + 1e-8 * max(1.0, float(np.abs(a).sum()))
    assert G.pairs_rest_at_a_bound(a, pairs, p.C)


# ---- (c) regression ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", G.WORKING_SETS)
@pytest.mark.parametrize("epsilon", [0.1, 0.0])
def test_real_valued_svr_trajectory_equals_the_twin_oracle(epsilon, q):
    X, z = G.real_svr()
    p = SVMParams(C=10.0, gamma=G.REAL_GAMMA, max_iter=10**7)
    Xd, mn, mx, K = _f64_problem(X, p.gamma)
    a2, res, tm = _svr_trajectory(Xd, mn, mx, K, z, p, epsilon, q=q, fp64_rows=True, cap=2100)
    assert tm["gram_path"] == "fp64"
    n = len(z)
    check_kkt(_torch_rbf(X, p.gamma), z, np.clip(a2[:n], 0.0, p.C), np.clip(a2[n:], 0.0, p.C), res.b, C=p.C,
              epsilon=epsilon, tau=p.tau)


@pytest.mark.parametrize("q", G.WORKING_SETS)
def test_pixel_svr_trajectory_equals_the_twin_oracle(q):
    X, z = G.pixel_svr()
    p = SVMParams()
    Xu, mn, mx, K = _u8_problem(X, p.gamma)
    a2, res, tm = _svr_trajectory(Xu, mn, mx, K, z, p, 0.05, q=q)
    assert tm["gram_path"] == "int8-exact"
    n = len(z)
    check_kkt(_torch_rbf(X, p.gamma), z, np.clip(a2[:n], 0.0, p.C), np.clip(a2[n:], 0.0, p.C), res.b, C=p.C,
              epsilon=0.05, tau=p.tau)


# ---- (d) heavily duplicated low-range integer data --------------------------------------------------------------
@SETTINGS
@given(G.low_range_strategy())
def test_low_range_integer_data_equals_the_oracle(prob):
    """4 - 256 distinct rows for 200 - 1500 points: every outer iteration's trace, alpha, b, iterations and the
    stop reason are the oracle's -- converged or max_iter, whichever the oracle reports -- the oracle's run
    floors, and a converged solve meets the stop test."""
    seed, n, d, vmax, Cb, gamma = prob
    X, y, _ = G.low_range_problem(seed, n, d, vmax)
    p = SVMParams(C=Cb, gamma=gamma)
    Xu, mn, mx, K = _u8_problem(X, gamma)
    yd = torch.from_numpy(y).to(DEV)
    alpha = torch.empty(n, dtype=torch.float64, device=DEV)
    cap = 1000  # outer iterations recorded on both sides (a longer solve is compared up to there, and at its end)
    dt = N.DecompTrace(cap, n)
    out = D.train_decomp(Xu, yd, alpha, p, mn, mx, trace=dt)
    assert out is not None
    res, tm = out
    a_o, r_o, st_o, ot = C.decomp_train_gram(K, y, p.replace(n_threads=8), trace_cap=cap, snapshots=True)
    assert st_o["eta_floor_updates"] > 0, "the inputs no longer reach the floored update"
    _compare(dt, ot)
    a = alpha.cpu().numpy()
    np.testing.assert_array_equal(a, a_o)
    assert (res.b, res.iterations, res.stop_reason) == (r_o.b, r_o.iterations, r_o.stop_reason)
    assert tm["outer_iterations"] == st_o["outer_iterations"]
    assert res.stop_reason in ("converged", "max_iter")
    if res.stop_reason == "converged":
        assert kkt_gap_fp64(X, y.astype(np.float64), a, p) <= 2 * p.tau + 1e-9


# ---- the estimators with default arguments ----------------------------------------------------------------------
def test_svc_with_default_arguments_converges():
    X, y, pairs = G.pixel_classifier(*G.PIXEL_SIZES[0])
    m = SVC(device="cuda:0").fit(X, y)
    assert m.stop_reason_ == "converged" and m.timings_["solver"] == "decomp"
    assert kkt_gap_fp64(X, y.astype(np.float64), m.alpha_, m.params) <= 2 * m.params.tau + 1e-9
    assert G.pairs_rest_at_a_bound(m.alpha_, pairs, m.params.C)
    Xr, yr, pr = G.real_classifier()
    m = SVC(gamma=G.REAL_GAMMA, device="cuda:0").fit(Xr, yr)
    assert m.stop_reason_ == "converged" and m.timings_["gram_path"] == "fp64"
    assert (kkt_gap_fp64(Xr, yr.astype(np.float64), m.alpha_, m.params)
            <= 2 * m.params.tau + 1e-8 * max(1.0, float(np.abs(m.alpha_).sum())))
    assert G.pairs_rest_at_a_bound(m.alpha_, pr, m.params.C)


def test_one_vs_rest_with_default_arguments_converges():
    """The copies carry a different class: each is a conflicting pair in two of the three one-vs-rest problems."""
    n, k = G.PIXEL_SIZES[0]
    ds = synthetic_mnist(n, seed=91).compact()
    lab = ds.labels % 3
    X = np.concatenate([ds.X, ds.X[:k]])
    labels = np.concatenate([lab, (lab[:k] + 1) % 3]).astype(np.int32)
    m = OneVsRestSVC(device="cuda:0").fit(X, labels, classes=[0, 1, 2])
    assert m.timings_["smo_solver"] == "decomp"
    assert list(m.stop_reasons_) == ["converged"] * 3
    for c in range(3):
        y = np.where(labels == c, 1, -1).astype(np.int32)
        s = SVC(device="cuda:0").fit(X, y)
        assert s.stop_reason_ == "converged" and m.intercepts_b_[c] == s.b_
        assert kkt_gap_fp64(X, y.astype(np.float64), s.alpha_, s.params) <= 2 * s.params.tau + 1e-9


def test_svr_with_default_arguments_converges():
    X, z = G.real_svr()
    m = SVR(gamma=G.REAL_GAMMA, device="cuda:0").fit(X, z)
    assert m.stop_reason_ == "converged" and m.timings_["gram_path"] == "fp64"
    check_kkt(_torch_rbf(X, G.REAL_GAMMA), z, m.alpha_, m.alpha_star_, m.b_, C=10.0, epsilon=0.1, tau=1e-5)
    Xp, zp = G.pixel_svr()
    m = SVR(epsilon=0.05, device="cuda:0").fit(Xp, zp)
    assert m.stop_reason_ == "converged" and m.timings_["gram_path"] == "int8-exact"
    check_kkt(_torch_rbf(Xp, G.PIXEL_GAMMA), zp, m.alpha_, m.alpha_star_, m.b_, C=10.0, epsilon=0.05, tau=1e-5)


# ---- scikit-learn fixtures --------------------------------------------------------------------------------------
def test_svr_fixture_predictions_on_the_gpu():
    g = G.load_fixture("svr_n240")
    m = SVR(C=g["C"], gamma=g["gamma"], epsilon=g["epsilon"], tol=1e-6, device="cuda:0", max_iter=10**7)
    m.fit(g["X"], g["z"])
    assert m.stop_reason_ == "converged"
    err = np.abs(m.predict(g["X"]) - g["pred"]).max()
    print(f"max |prediction - fixture| = {err:.3e} (bound {G.FIXTURE_SVR_TOL:.1e})")
    assert err <= G.FIXTURE_SVR_TOL


def test_svc_fixture_decision_values_on_the_gpu():
    g = G.load_fixture("svc_n330")
    m = SVC(C=g["C"], gamma=g["gamma"], tol=1e-6, device="cuda:0", max_iter=10**7).fit(g["X"], g["y"])
    assert m.stop_reason_ == "converged" and m.timings_["solver"] == "decomp"
    err = np.abs(m.decision_function(g["X"]) - g["dec"]).max()
    print(f"max |decision - fixture| = {err:.3e} (bound {G.FIXTURE_SVC_TOL:.1e})")
    assert err <= G.FIXTURE_SVC_TOL
    assert G.pairs_rest_at_a_bound(m.alpha_, g["pairs"], g["C"])


# ---- two ranks rehearsed on the one GPU -------------------------------------------------------------------------
def test_two_rank_rehearsal_equals_one_gpu():
    from svm355.parallel.decomp import DistributedDecompSVC
    from svm355.parallel.rccl import DeviceGroup

    X, y, pairs = G.pixel_classifier(*G.PIXEL_SIZES[1])
    one = SVC(device="cuda:0", solver="decomp").fit(X, y)
    g = DeviceGroup(2, "loopback")
    try:
        m = DistributedDecompSVC(2, group=g).fit(X, y)
    finally:
        g.close()
    assert m.stop_reason_ == one.stop_reason_ == "converged"
    assert m.n_iter_ == one.n_iter_ and m.b_ == one.b_
    np.testing.assert_array_equal(m.alpha_, one.alpha_)
    assert m.stats_["outer_iterations"] == one.timings_["outer_iterations"]
    assert G.pairs_rest_at_a_bound(m.alpha_, pairs, one.params.C)


# ---- the pairwise solver keeps the reference's rule -------------------------------------------------------------
def _pairwise_equals_its_oracle(X, y, p):
    _, _, _, K = _u8_problem(X, p.gamma)
    pw = SVC(C=p.C, gamma=p.gamma, device="cuda:0", solver="smo").fit(X, y)
    a_o, r_o, _ = C.smo_train_gram(K, y, p.replace(n_threads=8))
    np.testing.assert_array_equal(pw.alpha_, a_o)
    assert (pw.b_, pw.n_iter_, pw.stop_reason_) == (r_o.b, r_o.iterations, r_o.stop_reason)
    return pw.stop_reason_


def test_pairwise_solver_equals_the_pairwise_oracle_on_conflicting_copies():
    """The first-order choice takes the largest f, never the copy while it is violating: both converge."""
    X, y, _ = G.pixel_classifier(*G.PIXEL_SIZES[0])
    assert _pairwise_equals_its_oracle(X, y, SVMParams()) == "converged"
    g = G.load_fixture("svc_n330")
    assert _pairwise_equals_its_oracle(g["X"], g["y"], SVMParams(C=g["C"], gamma=g["gamma"])) == "converged"


@pytest.mark.parametrize("seed,n,d,vmax,Cb,gamma", [(0, 200, 2, 1, 1.0, 0.05), (3, 1200, 2, 3, 10.0, 0.00125)])
def test_pairwise_solver_keeps_the_reference_stop(seed, n, d, vmax, Cb, gamma):
    """Low-range data: many rows share the extreme f, the pair (i_high, i_low) is a pair of copies, and the
    reference stops ("non positive eta") -- on the device as in the oracle, after the same iterations."""
    X, y, _ = G.low_range_problem(seed, n, d, vmax)
    assert _pairwise_equals_its_oracle(X, y, SVMParams(C=Cb, gamma=gamma)) == "nonpositive_eta"
