"""epsilon-SVR on the device decomposition solver (twin mode, decomp.hip) against its CPU oracle
(``svm_decomp_train_gram_svr``, csrc/core/decomp_cpu.cpp) and against references of its own.

* The whole solve, bit for bit, given the device's own kernel values: every outer iteration's working set
  (virtual ids k / k + n), moved list, coefficients, inner iterations, bounds, the 2n alphas and the 2n f; on
  FP64 real rows (n = 300; n = 1,537 with working_set = 256: several selection blocks, several outer
  iterations, 2n not a multiple of 64), on uint8 pixel rows with a float target (the exact-integer plan), and
  on the same pixel rows with the column cache forced (SVM355_DECOMP_CCACHE=1: slots per row); an odd n; the
  cache under eviction, the streamed selection, the symmetric K(W, W), the inner solve's shapes and rules; twins
  of one row in different selection blocks (n = 1,537, working_set = 64).
* The fold + twin accumulate step alone, against the oracle's fold and its GEMV order applied to both halves.
* The KKT conditions of a GPU fit from a torch FP64 RBF (not the library's kernels), the scikit-learn
  fixture's predictions, and inference / persistence of device models (zero support vectors included).
"""

import numpy as np
import pytest
import torch

from svm355 import SVR, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C
from svm355.ops import device as D
from svm355.utils.data import synthetic_mnist

from svr_checks import FIXTURE_PRED_TOL, check_kkt, load_fixture, real_rows
from decomp_mode_checks import check_refusal, pixel_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


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
        np.testing.assert_array_equal(a["f"], b["f"], err_msg=f"outer {o}: f")
    return len(dr)


def _trajectory(Xdev, mn, mx, K, z, p, eps, q, fp64_rows=False, inner_wss=3, cap=400):
    n = z.shape[0]
    zd = torch.from_numpy(z).to(DEV)
    alpha = torch.empty(2 * n, dtype=torch.float64, device=DEV)
    dt = N.DecompTrace(cap, 2 * n)
    out = D.train_decomp_svr(Xdev, zd, alpha, p, mn, mx, epsilon=eps, working_set=q, trace=dt)
    assert out is not None
    res, tm = out
    a_o, r_o, st_o, ot = C.decomp_train_gram_svr(K, z, p.replace(n_threads=8), epsilon=eps, q=q, trace_cap=cap,
                                                 snapshots=True, fp64_rows=fp64_rows, inner_wss=inner_wss)
    outers = _compare(dt, ot)
    assert res.stop_reason == r_o.stop_reason == "converged"
    assert res.iterations == r_o.iterations and res.b == r_o.b
    np.testing.assert_array_equal(alpha.cpu().numpy(), a_o)
    assert tm["outer_iterations"] == st_o["outer_iterations"] == outers and tm["working_set"] == st_o["working_set"]
    return tm


@pytest.mark.parametrize("n,q,outers_at_least", [(300, 1024, 1), (1537, 256, 3)])
def test_fp64_rows_trajectory_equals_the_twin_oracle(n, q, outers_at_least):
    X, z = real_rows(n, seed=n)
    p = SVMParams(C=10.0, gamma=0.5, tau=1e-5)
    Xd = D.upload_rows(X, DEV)
    mn, mx, sqn = D.minmax_scale_(Xd, X.shape[1])
    nrm = D.row_norms(Xd, X.shape[1])  # the solve's own norms
    K = D.rbf_gram(Xd, nrm, Xd, nrm, p.gamma, symmetric=True)[:n, :n].cpu().numpy()
    tm = _trajectory(Xd, mn.cpu().numpy(), mx.cpu().numpy(), np.ascontiguousarray(K), z, p, 0.1, q, fp64_rows=True)
    assert tm["gram_path"] == "fp64" and tm["outer_iterations"] >= outers_at_least


@pytest.mark.parametrize("cache", [False, True])
def test_pixel_rows_trajectory_equals_the_twin_oracle(cache, monkeypatch):
    """uint8 pixel rows, a float target (the row's mean intensity / 16): the exact-integer plan; with the column
    cache forced, the cache holds one slot per row for both twins."""
    monkeypatch.setenv("SVM355_DECOMP_CCACHE", "1" if cache else "0")
    n = 2000
    tr = synthetic_mnist(n, seed=91).compact()
    z = np.ascontiguousarray(tr.X.astype(np.float64).mean(axis=1) / 16.0)
    Xu = D.upload_u8(tr.X, DEV)
    mmd = torch.empty(2 * tr.d, dtype=torch.float64, device=DEV)
    D.minmax_u8(Xu, out=mmd)
    mm = mmd.cpu().numpy()
    mn, mx = mm[: tr.d].copy(), mm[tr.d:].copy()
    Kd = D.rbf_gram_u8(Xu, 0.00125, mn, mx)
    assert Kd is not None
    K = np.ascontiguousarray(Kd[:n, :n].cpu().numpy())
    del Kd
    D.release_gram_buffers()
    tm = _trajectory(Xu, mn, mx, K, z, SVMParams(), 0.05, 1024)
    assert tm["gram_path"] == "int8-exact" and tm["outer_iterations"] >= 3


def _pixel_rows(n):
    """n uint8 pixel rows on the device, their column bounds, the float target (the row's mean intensity / 16) and
    the device's own exact-integer Gram on the host."""
    tr = synthetic_mnist(n, seed=91).compact()
    z = np.ascontiguousarray(tr.X.astype(np.float64).mean(axis=1) / 16.0)
    Xu = D.upload_u8(tr.X, DEV)
    mmd = torch.empty(2 * tr.d, dtype=torch.float64, device=DEV)
    D.minmax_u8(Xu, out=mmd)
    mm = mmd.cpu().numpy()
    mn, mx = mm[: tr.d].copy(), mm[tr.d:].copy()
    Kd = D.rbf_gram_u8(Xu, 0.00125, mn, mx)
    assert Kd is not None
    K = np.ascontiguousarray(Kd[:n, :n].cpu().numpy())
    del Kd
    D.release_gram_buffers()
    return Xu, mn, mx, K, z


@pytest.fixture(scope="module")
def pixel2000():
    return _pixel_rows(2000)


def test_odd_number_of_pixel_rows():
    """n = 1999: the twins' f update pairs rows (ws_cache_fsum_kernel<2, true>), and the last row has no partner."""
    Xu, mn, mx, K, z = _pixel_rows(1999)
    tm = _trajectory(Xu, mn, mx, K, z, SVMParams(), 0.05, 1024)
    assert tm["gram_path"] == "int8-exact" and tm["outer_iterations"] >= 3


# The decomposition solver's other paths in twin mode (the classifier's tests run them in test_gpu_decomp_oracle.py):
# the column cache under eviction (300 slots: the cache fills and the CLOCK sweep evicts; 8: the hand wraps, most
# misses take scratch slots), the streamed selection, K(W, W) from the triangular Gram launch, the inner solve's
# workgroup shapes and selection rules (the oracle reads SVM355_DECOMP_NT and takes inner_wss).
@pytest.mark.parametrize("env,inner_wss", [({"SVM355_DECOMP_CCACHE": "1", "SVM355_DECOMP_CCACHE_SLOTS": "300"}, 3),
                                           ({"SVM355_DECOMP_CCACHE": "1", "SVM355_DECOMP_CCACHE_SLOTS": "8"}, 3),
                                           ({"SVM355_DECOMP_WIDE_SELECT": "1"}, 3),
                                           ({"SVM355_DECOMP_KWW": "sym"}, 3),
                                           ({"SVM355_DECOMP_NT": "64"}, 3),
                                           ({"SVM355_DECOMP_NT": "128"}, 3),
                                           ({"SVM355_DECOMP_NT": "512"}, 3),
                                           ({"SVM355_DECOMP_WSS": "1"}, 1),
                                           ({"SVM355_DECOMP_WSS": "2"}, 2),
                                           ({"SVM355_DECOMP_WSS": "4"}, 4)],
                         ids=lambda v: "-".join(f"{k[14:]}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_twin_mode_paths_equal_the_twin_oracle(pixel2000, env, inner_wss, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    Xu, mn, mx, K, z = pixel2000
    tm = _trajectory(Xu, mn, mx, K, z, SVMParams(), 0.05, 1024, inner_wss=inner_wss)
    assert tm["gram_path"] == "int8-exact" and tm["outer_iterations"] >= 3
    if "SVM355_DECOMP_NT" in env:
        assert tm["inner_threads"] == int(env["SVM355_DECOMP_NT"])


def test_twins_of_one_row_in_different_selection_blocks():
    """n = 1,537 real rows, q = 64: the 2n = 3,074 virtual points fall into 56 selection blocks of 55, one
    candidate pair per block and working set (112 slots), so a row's twins (k and k + 1,537) lie in different
    blocks and the solve takes hundreds of outer iterations."""
    n = 1537
    X, z = real_rows(n, seed=n)
    p = SVMParams(C=10.0, gamma=0.5, tau=1e-5)
    Xd = D.upload_rows(X, DEV)
    mn, mx, sqn = D.minmax_scale_(Xd, X.shape[1])
    nrm = D.row_norms(Xd, X.shape[1])
    K = D.rbf_gram(Xd, nrm, Xd, nrm, p.gamma, symmetric=True)[:n, :n].cpu().numpy()
    tm = _trajectory(Xd, mn.cpu().numpy(), mx.cpu().numpy(), np.ascontiguousarray(K), z, p, 0.1, 64, fp64_rows=True,
                     cap=800)
    assert tm["gram_path"] == "fp64" and tm["working_set"] == 112 and tm["outer_iterations"] >= 100


@pytest.mark.parametrize("via", ["gemv", "cache"])
def test_fold_and_twin_accumulate_step(via, monkeypatch):
    """n = 130 rows (a partial row tile): a moved list with both twins of some rows (in both orders) and lone
    twins; the device's folded update of the 2n f equals the oracle's fold + its GEMV order on both halves."""
    monkeypatch.setenv("SVM355_GEMV_VIA_CACHE", "1" if via == "cache" else "0")
    n = 130
    tr = synthetic_mnist(n, seed=17).compact()
    Xu = D.upload_u8(tr.X, DEV)
    mmd = torch.empty(2 * tr.d, dtype=torch.float64, device=DEV)
    D.minmax_u8(Xu, out=mmd)
    mm = mmd.cpu().numpy()
    mn, mx = mm[: tr.d].copy(), mm[tr.d:].copy()
    K = np.ascontiguousarray(D.rbf_gram_u8(Xu, 0.00125, mn, mx)[:n, :n].cpu().numpy())
    rng = np.random.default_rng(3)
    both = rng.choice(n, size=40, replace=False)
    lone = np.setdiff1d(np.arange(n), both)[:30]
    cols = np.concatenate([both[:20], both[:20] + n, both[20:] + n, both[20:], lone[:15], lone[15:] + n])
    cols = cols[rng.permutation(cols.size)].astype(np.int32)
    coef = rng.uniform(-10.0, 10.0, size=cols.size)
    f0 = rng.normal(size=2 * n)
    out = D.decomp_twin_step_u8(Xu, mn, mx, 0.00125, cols, coef, f0)
    assert out is not None
    rows, rc = C.twin_fold(cols, coef, n)
    assert rows.size == 70 and np.unique(rows).size == 70
    ref = f0.copy()
    for half in (ref[:n], ref[n:]):  # views: the oracle's gemv_update on each half
        N.check(N.core().svm_decomp_gemv_ref(N.ptr(K), K.shape[1], n, N.ptr(rows), N.ptr(rc), rows.size, N.ptr(half)),
                "svm_decomp_gemv_ref")
    np.testing.assert_array_equal(out, ref)
    assert np.abs(out[:n] - f0[:n] - K[:, rows] @ rc).max() < 1e-11


def test_kkt_of_a_gpu_fit_from_a_torch_rbf():
    n = 2000
    X, z = real_rows(n, seed=5)
    m = SVR(C=10.0, gamma=0.5, epsilon=0.1, tol=1e-5, device="cuda:0", max_iter=10**7).fit(X, z)
    assert m.stop_reason_ == "converged" and m.timings_["gram_path"] == "fp64"
    Xt = torch.from_numpy(X).to(DEV)
    d2 = torch.cdist(Xt, Xt, compute_mode="donot_use_mm_for_euclid_dist") ** 2
    K = torch.exp(-0.5 * d2).cpu().numpy()
    check_kkt(K, z, m.alpha_, m.alpha_star_, m.b_, C=10.0, epsilon=0.1, tau=1e-5)


@pytest.mark.parametrize("seed", [11, 12])
def test_fixture_predictions_on_the_gpu(seed):
    g = load_fixture(seed)
    m = SVR(C=g["C"], gamma=g["gamma"], epsilon=g["epsilon"], tol=1e-6, device="cuda:0", max_iter=10**7)
    m.fit(g["X"], g["z"])
    assert m.stop_reason_ == "converged"
    np.testing.assert_array_equal(m.scaler_.min_, 0.0)  # the fixture's rows: scaling is the identity
    np.testing.assert_array_equal(m.scaler_.max_, 1.0)
    assert np.abs(m.predict(g["X"]) - g["pred"]).max() <= FIXTURE_PRED_TOL


def test_predict_score_and_persistence_on_the_device(tmp_path):
    X, z = real_rows(400, seed=9)
    Xq, zq = real_rows(150, seed=10, bounds_of=X)
    m = SVR(C=10.0, gamma=0.5, epsilon=0.1, device="cuda:0").fit(X, z)
    beta = m.alpha_ - m.alpha_star_
    d2 = ((Xq[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    ref = np.exp(-0.5 * d2) @ beta - m.b_
    pred = m.predict(Xq)
    assert np.abs(pred - ref).max() < 1e-10
    r2 = 1.0 - ((zq - ref) ** 2).sum() / ((zq - zq.mean()) ** 2).sum()
    assert abs(m.score(Xq, zq) - r2) < 1e-9 and r2 > 0.8
    m.save(tmp_path / "m")
    back = SVR.load(tmp_path / "m", device="cuda:0")
    np.testing.assert_array_equal(back.predict(Xq), pred)
    np.testing.assert_array_equal(back.support_, m.support_)


def test_zero_support_vector_model_predicts_on_the_device(tmp_path):
    X, z = real_rows(64, seed=2)
    z = 0.5 + 0.1 * (z - z.min()) / (z.max() - z.min())  # spread 0.1 <= 2 epsilon
    m = SVR(epsilon=0.05, gamma=0.5, device="cuda:0").fit(X, z)
    assert len(m.support_) == 0 and m.n_iter_ == 1 and m.timings_["outer_iterations"] == 0
    np.testing.assert_array_equal(m.predict(X[:5]), np.full(5, (z.max() + z.min()) / 2))
    m.save(tmp_path / "z")
    np.testing.assert_array_equal(SVR.load(tmp_path / "z", device="cuda:0").predict(X[:5]), m.predict(X[:5]))


def test_gpu_refusals(monkeypatch):
    X, z = real_rows(64, seed=2)
    with pytest.raises(ValueError, match="scale=True"):
        SVR(scale=False, device="cuda:0").fit(X, z)
    Xd = D.upload_rows(X, DEV)
    mn, mx, _ = D.minmax_scale_(Xd, X.shape[1])
    zd = torch.from_numpy(z).to(DEV)
    alpha = torch.empty(128, dtype=torch.float64, device=DEV)
    for p, what in ((SVMParams(shrinking=True), "shrinking"), (SVMParams(weight_pos=2.0), "class weights")):
        with pytest.raises(N.NativeError, match=what):
            D.train_decomp_svr(Xd, zd, alpha, p, mn.cpu().numpy(), mx.cpu().numpy())
    with pytest.raises(N.NativeError, match="epsilon"):
        D.train_decomp_svr(Xd, zd, alpha, SVMParams(), mn.cpu().numpy(), mx.cpu().numpy(), epsilon=-0.1)
    monkeypatch.setenv("SVM355_DECOMP_NEWTON", "1")
    with pytest.raises(N.NativeError, match="Newton"):
        D.train_decomp_svr(Xd, zd, alpha, SVMParams(), mn.cpu().numpy(), mx.cpu().numpy())


@pytest.mark.parametrize("feature", ["shrinking", "newton", "weights"])
def test_entry_refuses_under_its_name_and_enqueues_nothing(feature, monkeypatch):
    rows = pixel_rows(DEV)
    z = torch.linspace(0.0, 1.0, 64, dtype=torch.float64, device=DEV)
    alpha = torch.empty(128, dtype=torch.float64, device=DEV)
    check_refusal("svmd_train_decomp_svr", "regression (twin)", feature,
                  lambda p: D.train_decomp_svr(rows[0], z, alpha, p, rows[1], rows[2]), rows, monkeypatch)
