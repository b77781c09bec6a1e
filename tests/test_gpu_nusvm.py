"""nu-SVC and nu-SVR on the device decomposition solver's nu modes (csrc/hip/decomp_nu.hip) against the CPU oracle
(csrc/core/decomp_cpu.cpp) and against references of their own.

* The whole solve, bit for bit, given the device's own kernel values: every outer iteration's working set, moved
  list, coefficients, inner iterations, bounds, alpha and f -- FP64 rows at (n, q) = (300, 1024) and (1537, 256: 32
  blocks, 2 picks per list), pixel rows with the column cache off and forced, nu-SVC's start at the chunk edge.
* The KKT conditions of default GPU fits from a torch FP64 RBF (not the library's kernels), also with a working set
  smaller than one wave; the equivalence with SVC(C = 1 / r_); inference, persistence and the refusals.
"""
import numpy as np
import pytest
import torch

from svm355 import SVC, NuSVC, NuSVR, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C
from svm355.ops import device as D
from svm355.utils.data import synthetic_mnist

from decomp_mode_checks import check_refusal, pixel_rows
from nusvm_checks import SHAPES, SVC_EQUIV_TOL, compare_traces, kkt_nusvc, kkt_nusvr, labels, nusvc_case
from svr_checks import real_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = ("nusvc", "nusvr")


def _trajectory(kind, Xdev, mn, mx, K, target, p, nu, q, fp64_rows, cap=400):
    """The device solve and the oracle on the device's own kernel values K, compared record by record."""
    n = K.shape[0]
    points = n if kind == "nusvc" else 2 * n
    alpha = torch.empty(points, dtype=torch.float64, device=DEV)
    dt = N.DecompTrace(cap, points)
    td = torch.from_numpy(target).to(DEV)
    out = (D.train_decomp_nusvc if kind == "nusvc" else D.train_decomp_nusvr)(Xdev, td, alpha, p, mn, mx, nu=nu,
                                                                               working_set=q, trace=dt)
    assert out is not None
    res, tm, rr = out
    oracle = C.decomp_train_gram_nusvc if kind == "nusvc" else C.decomp_train_gram_nusvr
    a_o, r_o, st_o, rr_o, ot = oracle(K, target, p.replace(n_threads=8), nu=nu, q=q, trace_cap=cap, snapshots=True,
                                      fp64_rows=fp64_rows)
    outers = compare_traces(dt, ot)
    assert res.stop_reason == r_o.stop_reason == "converged"
    assert res.iterations == r_o.iterations and res.b == r_o.b and rr == rr_o
    np.testing.assert_array_equal(alpha.cpu().numpy(), a_o)
    assert tm["outer_iterations"] == st_o["outer_iterations"] == outers and tm["working_set"] == st_o["working_set"]
    return tm


def _fp64_rows(n, seed):
    """n real rows scaled on the device (the identity), the targets, and the device's own FP64 Gram on the host."""
    X, z = real_rows(n, seed=seed)
    Xd = D.upload_rows(X, DEV)
    mn, mx, _ = D.minmax_scale_(Xd, X.shape[1])
    nrm = D.row_norms(Xd, X.shape[1])  # the solve's own norms
    K = D.rbf_gram(Xd, nrm, Xd, nrm, 0.5, symmetric=True)[:n, :n].cpu().numpy()
    return X, z, Xd, mn.cpu().numpy(), mx.cpu().numpy(), np.ascontiguousarray(K)


def _target(kind, X, z):
    return labels(X, z)[1] if kind == "nusvc" else z


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,q,outers_at_least", [(*SHAPES[0], 1), (*SHAPES[1], 3)])
def test_fp64_rows_trajectory_equals_the_oracle(kind, n, q, outers_at_least):
    X, z, Xd, mn, mx, K = _fp64_rows(n, seed=n)
    tm = _trajectory(kind, Xd, mn, mx, K, _target(kind, X, z), SVMParams(gamma=0.5, tau=1e-5, C=2.0), 0.4, q, True)
    assert tm["gram_path"] == "fp64" and tm["outer_iterations"] >= outers_at_least


@pytest.mark.parametrize("cache", [False, True])
def test_pixel_rows_trajectory_equals_the_oracle(cache, monkeypatch):
    """uint8 pixel rows: the exact-integer plan; with the column cache forced, the start's columns are its first
    stores."""
    monkeypatch.setenv("SVM355_DECOMP_CCACHE", "1" if cache else "0")
    n = 2000
    tr = synthetic_mnist(n, seed=91).compact()
    y = tr.y.astype(np.int32)  # one digit against the rest: about 1 : 9
    nu = min((y == 1).sum(), (y == -1).sum()) / n  # half of nu_max
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
    tm = _trajectory("nusvc", Xu, mn, mx, K, y, SVMParams(gamma=0.00125), nu, 1024, False)
    assert tm["gram_path"] == "int8-exact" and tm["outer_iterations"] >= 1


def test_nusvc_start_across_the_chunk_edge():
    """The start is summed in chunks of 1,024 columns.  Both classes get nu n / 2, so the start has 2 ceil(nu n / 2)
    columns -- an even number: 1,025 cannot occur, and 1,026 is the first count past the edge (n = 2,050, nu = 0.5:
    512 ones and a half per class; the second chunk holds two columns)."""
    n = 2050
    X, z, Xd, mn, mx, K = _fp64_rows(n, seed=n)
    tm = _trajectory("nusvc", Xd, mn, mx, K, labels(X, z)[1], SVMParams(gamma=0.5, tau=1e-5), 0.5, 1024, True)
    assert tm["start_columns"] == 1026 and tm["gram_path"] == "fp64"


def _torch_rbf(X, gamma, rows=1024):
    """The reference kernel matrix: torch's FP64 cdist, 1,024 rows at a time; checked itself (unit diagonal,
    symmetry)."""
    Xt = torch.from_numpy(X).to(DEV)
    K = torch.empty((len(X), len(X)), dtype=torch.float64, device=DEV)
    for i in range(0, len(X), rows):
        d2 = torch.cdist(Xt[i:i + rows], Xt, compute_mode="donot_use_mm_for_euclid_dist") ** 2
        K[i:i + rows] = torch.exp(-gamma * d2)
    K = K.cpu().numpy()
    assert np.all(np.diag(K) == 1.0) and np.abs(K - K.T).max() <= 1e-14 and K[-1, 0] < 1.0
    return K


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,q", [(2000, 1024), (40, 32)])
def test_kkt_of_gpu_fits_from_a_torch_rbf(kind, n, q):
    X, z = real_rows(n, seed=5)
    kw = dict(nu=0.3, gamma=0.5, tol=1e-5, device="cuda:0", max_iter=10**7, working_set=q)
    K = _torch_rbf(X, 0.5)
    if kind == "nusvc":
        y = labels(X, z)[1]
        m = NuSVC(**kw).fit(X, y)
        a = np.zeros(n)
        a[m.support_] = np.abs(m.dual_coef_)
        kkt_nusvc(K, y, a, m.r_, m.rho_, 0.3, 1e-5)
    else:
        m = NuSVR(C=2.0, **kw).fit(X, z)
        kkt_nusvr(K, z, np.concatenate([m.alpha_, m.alpha_star_]), 2.0, m.r_, m.rho_, 0.3, 1e-5)
        assert m.epsilon_ == -m.r_ > 0
    assert m.stop_reason_ == "converged" and m.timings_["gram_path"] == "fp64"


def test_nusvc_equals_svc_at_c_one_over_r_on_the_gpu():
    """test_nusvm_cpu.py's case (where SVC_EQUIV_TOL was measured), both fits on the device."""
    X, y = nusvc_case(300, seed=7)
    Xq, _ = real_rows(200, seed=8, bounds_of=X)
    kw = dict(gamma=0.5, tol=1e-5, device="cuda:0", max_iter=10**7)
    nu = NuSVC(nu=0.4, **kw).fit(X, y)
    svc = SVC(C=1.0 / nu.r_, solver="decomp", **kw).fit(X, y)
    diff = np.abs(nu.decision_function(Xq) - svc.decision_function(Xq)).max()
    print(f"max |NuSVC - SVC(1 / r)| decision on held-out rows = {diff:.3e} (bound {SVC_EQUIV_TOL:.3e})")
    assert nu.stop_reason_ == svc.stop_reason_ == "converged" and diff <= SVC_EQUIV_TOL


@pytest.mark.parametrize("kind", KINDS)
def test_decision_predict_and_persistence_on_the_device(kind, tmp_path):
    X, z = real_rows(400, seed=9)
    Xq, _ = real_rows(150, seed=10, bounds_of=X)
    kw = dict(nu=0.3, gamma=0.5, device="cuda:0")
    if kind == "nusvc":
        y = labels(X, z)[1]
        m = NuSVC(**kw).fit(X, y)
        coef, out = m.alpha_ * y, m.decision_function(Xq)
        np.testing.assert_array_equal(m.predict(Xq), np.where(out > 0, 1, -1))
        assert m.intercept_ == -m.rho_ / m.r_ == -m.b_ and 0.5 < m.score(X, y) <= 1.0
    else:
        m = NuSVR(C=2.0, **kw).fit(X, z)
        coef, out = m.alpha_ - m.alpha_star_, m.predict(Xq)
        assert m.intercept_ == -m.rho_ == -m.b_ and m.score(X, z) > 0.8
    d2 = ((Xq[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    assert np.abs(out - (np.exp(-0.5 * d2) @ coef - m.b_)).max() < 1e-10
    m.save(tmp_path / "m")
    back = type(m).load(tmp_path / "m", device="cuda:0")
    np.testing.assert_array_equal(back._decision(Xq), out)
    np.testing.assert_array_equal(back.support_, m.support_)
    with pytest.raises(ValueError, match=kind):
        (NuSVR if kind == "nusvc" else NuSVC).load(tmp_path / "m")


def _call(kind, rows, alpha, z, **kw):
    if kind == "nusvc":
        return lambda p: D.train_decomp_nusvc(rows[0], rows[3], alpha, p, rows[1], rows[2], **kw)
    return lambda p: D.train_decomp_nusvr(rows[0], z, alpha, p, rows[1], rows[2], **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("feature", ["shrinking", "newton", "weights"])
def test_entry_refuses_under_its_name_and_enqueues_nothing(kind, feature, monkeypatch):
    rows = pixel_rows(DEV)
    alpha = torch.empty(64 if kind == "nusvc" else 128, dtype=torch.float64, device=DEV)
    z = torch.linspace(0, 1, 64, dtype=torch.float64, device=DEV)
    check_refusal(f"svmd_train_decomp_{kind}", "nu-SVC" if kind == "nusvc" else "nu-SVR", feature,
                  _call(kind, rows, alpha, z, nu=0.3), rows, monkeypatch)


@pytest.mark.parametrize("kind", KINDS)
def test_gpu_refusals_of_the_mode_s_own_arguments(kind):
    X, z = real_rows(64, seed=2)
    with pytest.raises(ValueError, match="scale=True"):
        (NuSVC if kind == "nusvc" else NuSVR)(scale=False, device="cuda:0").fit(X, labels(X, z)[1] if kind == "nusvc" else z)
    rows = pixel_rows(DEV)
    alpha = torch.empty(64 if kind == "nusvc" else 128, dtype=torch.float64, device=DEV)
    zd = torch.from_numpy(z).to(DEV)
    for nu in (0.0, 1.5, -0.2, float("nan")):
        with pytest.raises(N.NativeError, match=r"nu must be in \(0, 1\]"):
            _call(kind, rows, alpha, zd, nu=nu)(SVMParams(gamma=0.5))
    if kind == "nusvc":  # 32 : 32 labels, and a count that says 8 : 56
        with pytest.raises(N.NativeError, match="specified nu is infeasible"):
            _call(kind, rows, alpha, zd, nu=0.5, n_pos=8)(SVMParams(gamma=0.5))
    # the point cap, refused by name before any device work: 1,048,577 points (nu-SVR: 2 n)
    n = 1048577 if kind == "nusvc" else 524289
    Xu = torch.zeros((n, 16), dtype=torch.uint8, device=DEV)
    big = torch.empty(1048577 if kind == "nusvc" else 2 * n, dtype=torch.float64, device=DEV)
    tgt = torch.ones(n, dtype=torch.int32, device=DEV) if kind == "nusvc" else torch.zeros(n, dtype=torch.float64, device=DEV)
    with pytest.raises(N.NativeError, match="at most 1048576 points"):
        _call(kind, (Xu, rows[1], rows[2], tgt), big, tgt, nu=0.3, **({"n_pos": n // 2} if kind == "nusvc" else {}))(
            SVMParams(gamma=0.5))


