"""One-class SVM on the device decomposition solver (one-class mode, decomp.hip) against its CPU oracle
(``svm_decomp_train_gram_oneclass``, csrc/core/decomp_cpu.cpp) and against references of its own.

* The whole solve, bit for bit, given the device's own kernel values: every outer iteration's working set, moved
  list, coefficients, inner iterations, bounds, alpha and f; on FP64 real rows (n = 300; n = 1,537 with
  working_set = 256: several selection blocks, several outer iterations, n not a multiple of 64) and on uint8
  pixel rows (the exact-integer plan) with the column cache off and forced.
* The start's chunk edges: 1,023 / 1,024 / 1,025 start columns (one chunk, a full chunk, a second chunk of one
  column) and exactly 1,024 ones without a fractional point; the compaction across its 8,192-point pass.
* The KKT conditions of GPU fits from a torch FP64 RBF (not the library's kernels), the scikit-learn fixtures'
  decision values, inference and persistence of device models, and the refusals.
"""

import numpy as np
import pytest
import torch

from svm355 import OneClassSVM, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C
from svm355.ops import device as D
from svm355.utils.data import synthetic_mnist

from decomp_mode_checks import check_refusal, pixel_rows
from oneclass_checks import FIXTURE_DEC_TOL, FIXTURES, check_kkt, load_fixture
from svr_checks import real_rows

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


def _trajectory(Xdev, mn, mx, K, p, nu, q, fp64_rows=False, cap=400):
    n = K.shape[0]
    alpha = torch.empty(n, dtype=torch.float64, device=DEV)
    dt = N.DecompTrace(cap, n)
    out = D.train_decomp_oneclass(Xdev, alpha, p, mn, mx, nu=nu, working_set=q, trace=dt)
    assert out is not None
    res, tm = out
    a_o, r_o, st_o, ot = C.decomp_train_gram_oneclass(K, p.replace(n_threads=8), nu=nu, q=q, trace_cap=cap,
                                                      snapshots=True, fp64_rows=fp64_rows)
    assert tm["start_columns"] == st_o["start_columns"]
    np.testing.assert_array_equal(dt.records()[0]["bounds"], ot.records()[0]["bounds"])  # the start's f
    outers = _compare(dt, ot)
    assert res.stop_reason == r_o.stop_reason == "converged"
    assert res.iterations == r_o.iterations and res.b == r_o.b
    np.testing.assert_array_equal(alpha.cpu().numpy(), a_o)
    assert tm["outer_iterations"] == st_o["outer_iterations"] == outers and tm["working_set"] == st_o["working_set"]
    return tm


def _fp64_rows(n, seed):
    """n real rows scaled on the device (the identity), and the device's own FP64 Gram on the host."""
    X, _ = real_rows(n, seed=seed)
    Xd = D.upload_rows(X, DEV)
    mn, mx, _ = D.minmax_scale_(Xd, X.shape[1])
    nrm = D.row_norms(Xd, X.shape[1])  # the solve's own norms
    K = D.rbf_gram(Xd, nrm, Xd, nrm, 0.5, symmetric=True)[:n, :n].cpu().numpy()
    return Xd, mn.cpu().numpy(), mx.cpu().numpy(), np.ascontiguousarray(K)


@pytest.mark.parametrize("n,q,outers_at_least", [(300, 1024, 1), (1537, 256, 3)])
def test_fp64_rows_trajectory_equals_the_oracle(n, q, outers_at_least):
    Xd, mn, mx, K = _fp64_rows(n, seed=n)
    tm = _trajectory(Xd, mn, mx, K, SVMParams(gamma=0.5, tau=1e-5), 0.2, q, fp64_rows=True)
    assert tm["gram_path"] == "fp64" and tm["outer_iterations"] >= outers_at_least
    assert tm["start_columns"] == {300: 60, 1537: 308}[n]  # 0.2 n = 60 (no fractional point) and 307.4


@pytest.mark.parametrize("cache", [False, True])
def test_pixel_rows_trajectory_equals_the_oracle(cache, monkeypatch):
    """uint8 pixel rows: the exact-integer plan; with the column cache forced, the start's columns are its first
    stores (200 columns of one f update: the tiled store)."""
    monkeypatch.setenv("SVM355_DECOMP_CCACHE", "1" if cache else "0")
    n = 2000
    tr = synthetic_mnist(n, seed=91).compact()
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
    tm = _trajectory(Xu, mn, mx, K, SVMParams(gamma=0.00125), 0.1, 1024)
    assert tm["gram_path"] == "int8-exact" and tm["outer_iterations"] >= 1 and tm["start_columns"] == 200


# The start is summed in chunks of 1,024 columns (nz_update): one short of a chunk, a full chunk, one column into
# a second chunk, and a full chunk of ones with no fractional point after it.
@pytest.mark.parametrize("n,nu,columns", [(2050, 1022.5 / 2050, 1023), (2050, 1023.5 / 2050, 1024),
                                          (2050, 1024.5 / 2050, 1025), (2048, 0.5, 1024)])
def test_start_chunk_edges(n, nu, columns):
    Xd, mn, mx, K = _fp64_rows(n, seed=n)
    tm = _trajectory(Xd, mn, mx, K, SVMParams(gamma=0.5, tau=1e-5), nu, 1024, fp64_rows=True)
    assert tm["start_columns"] == columns and tm["gram_path"] == "fp64"


def _torch_rbf(X, gamma, rows=1024):
    """The reference kernel matrix: torch's FP64 cdist, 1,024 rows at a time (its direct kernel launches one
    workgroup per output, and one launch over all of 8,500 x 8,500 outputs left the last rows unwritten).  The
    reference is checked itself: a unit diagonal and symmetry."""
    Xt = torch.from_numpy(X).to(DEV)
    K = torch.empty((len(X), len(X)), dtype=torch.float64, device=DEV)
    for i in range(0, len(X), rows):
        d2 = torch.cdist(Xt[i:i + rows], Xt, compute_mode="donot_use_mm_for_euclid_dist") ** 2
        K[i:i + rows] = torch.exp(-gamma * d2)
    K = K.cpu().numpy()
    assert np.all(np.diag(K) == 1.0) and np.abs(K - K.T).max() <= 1e-14 and K[-1, 0] < 1.0
    return K


def test_compaction_across_its_8192_point_pass():
    """n = 8,500, nu = 0.98: 8,330 start columns -- the compaction kernel's second pass of 8,192 points and 9
    chunks of the start."""
    n, nu = 8500, 0.98
    X, _ = real_rows(n, seed=41)
    m = OneClassSVM(nu=nu, gamma=0.5, tol=1e-5, device="cuda:0", max_iter=10**7).fit(X)
    assert m.stop_reason_ == "converged" and m.timings_["gram_path"] == "fp64"
    assert m.timings_["start_columns"] == 8330
    check_kkt(_torch_rbf(X, 0.5), m.alpha_, m.rho_, nu, tau=1e-5)


def test_kkt_of_a_default_gpu_fit_from_a_torch_rbf():
    n, nu = 2000, 0.1
    X, _ = real_rows(n, seed=5)
    m = OneClassSVM(nu=nu, gamma=0.5, tol=1e-5, device="cuda:0", max_iter=10**7).fit(X)
    assert m.stop_reason_ == "converged" and m.timings_["gram_path"] == "fp64"
    check_kkt(_torch_rbf(X, 0.5), m.alpha_, m.rho_, nu, tau=1e-5)


@pytest.mark.parametrize("n,seed", FIXTURES)
def test_fixture_decisions_on_the_gpu(n, seed):
    g = load_fixture(n, seed)
    m = OneClassSVM(nu=g["nu"], gamma=g["gamma"], tol=1e-6, device="cuda:0", max_iter=10**7).fit(g["X"])
    assert m.stop_reason_ == "converged"
    np.testing.assert_array_equal(m.scaler_.min_, 0.0)  # the fixture's rows: scaling is the identity
    np.testing.assert_array_equal(m.scaler_.max_, 1.0)
    err = np.abs(m.decision_function(g["X"]) - g["decision"]).max()
    print(f"seed {seed}: max |decision - fixture| = {err:.3e}, |rho - fixture| = {abs(m.rho_ - g['rho']):.3e} "
          f"(bound {FIXTURE_DEC_TOL:.3e})")
    assert err <= FIXTURE_DEC_TOL
    assert abs(m.rho_ - g["rho"]) <= FIXTURE_DEC_TOL


def test_decision_predict_and_persistence_on_the_device(tmp_path):
    X, _ = real_rows(400, seed=9)
    Xq, _ = real_rows(150, seed=10, bounds_of=X)
    Xq = np.vstack([Xq, Xq[:5] + 3.0])  # far outside the training range: outliers
    m = OneClassSVM(nu=0.2, gamma=0.5, device="cuda:0").fit(X)
    d2 = ((Xq[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    ref = np.exp(-0.5 * d2) @ m.alpha_ - m.rho_
    dec = m.decision_function(Xq)
    assert np.abs(dec - ref).max() < 1e-10
    pred = m.predict(Xq)
    np.testing.assert_array_equal(pred, np.where(dec > 0, 1, -1))
    assert pred.dtype.kind == "i" and set(np.unique(pred)) == {-1, 1} and np.all(pred[-5:] == -1)
    np.testing.assert_array_equal(m.score_samples(Xq), dec + m.rho_)
    np.testing.assert_allclose(m.score_samples(Xq) - dec, m.rho_, rtol=0, atol=1e-12)  # a rounding of rho + dec
    assert m.b_ == m.rho_ == m.offset_ == -m.intercept_
    m.save(tmp_path / "m")
    back = OneClassSVM.load(tmp_path / "m", device="cuda:0")
    np.testing.assert_array_equal(back.predict(Xq), pred)
    np.testing.assert_array_equal(back.decision_function(Xq), dec)
    np.testing.assert_array_equal(back.support_, m.support_)


def test_gpu_refusals(monkeypatch):
    X, _ = real_rows(64, seed=2)
    with pytest.raises(ValueError, match="scale=True"):
        OneClassSVM(scale=False, device="cuda:0").fit(X)
    Xd = D.upload_rows(X, DEV)
    mn, mx, _ = D.minmax_scale_(Xd, X.shape[1])
    mn, mx = mn.cpu().numpy(), mx.cpu().numpy()
    alpha = torch.empty(64, dtype=torch.float64, device=DEV)
    for p, what in ((SVMParams(shrinking=True), "shrinking"), (SVMParams(weight_pos=2.0), "class weights")):
        with pytest.raises(N.NativeError, match=what):
            D.train_decomp_oneclass(Xd, alpha, p, mn, mx, nu=0.3)
    for nu in (0.0, 1.0, -0.2, float("nan")):
        with pytest.raises(N.NativeError, match="nu"):
            D.train_decomp_oneclass(Xd, alpha, SVMParams(), mn, mx, nu=nu)
    monkeypatch.setenv("SVM355_DECOMP_NEWTON", "1")
    with pytest.raises(N.NativeError, match="Newton"):
        D.train_decomp_oneclass(Xd, alpha, SVMParams(), mn, mx, nu=0.3)


@pytest.mark.parametrize("feature", ["shrinking", "newton", "weights"])
def test_entry_refuses_under_its_name_and_enqueues_nothing(feature, monkeypatch):
    rows = pixel_rows(DEV)
    alpha = torch.empty(64, dtype=torch.float64, device=DEV)
    check_refusal("svmd_train_decomp_oneclass", "one-class", feature,
                  lambda p: D.train_decomp_oneclass(rows[0], alpha, p, rows[1], rows[2], nu=0.3), rows, monkeypatch)
