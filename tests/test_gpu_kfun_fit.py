"""SVC / SVR with the linear, polynomial and sigmoid kernels on the GPU decomposition solver: the device trajectory
against the CPU oracle on the device's own kernel values, optimality from an independent numpy Gram, prediction,
the scikit-learn fixture, and the refusals."""
import numpy as np
import pytest
import torch

from svm355 import SVC, SVR, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C
from svm355.ops import device as D

from kfun_checks import C as BOX, EPSILON, FIXTURE_TOL, KERNELS, TANH_DEV, U, kernel_ref, load_fixture, rows_labels_targets
from test_gpu_decomp_oracle import _compare

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WEIGHTS = {1: 2.0, -1: 0.5}


def _rows(X):
    rows = D.upload_rows(X, DEV)
    mm = D.minmax_scale_(rows, X.shape[1])
    return rows, mm[0].cpu().numpy(), mm[1].cpu().numpy()


@pytest.mark.parametrize("est", ["svc", "svc_weighted", "svr"])
@pytest.mark.parametrize("n,q", [(300, 64), (300, 1024), (1537, 256)])
@pytest.mark.parametrize("name", list(KERNELS))
def test_trajectory_equals_the_oracle_and_the_fit_is_optimal(name, n, q, est):
    X, y, z = rows_labels_targets(n, 7 + n)
    w = WEIGHTS if est == "svc_weighted" else {1: 1.0, -1: 1.0}
    # max_iter: the polynomial SVR at q = 256 takes more than the default 100,000 pair updates
    p = SVMParams(C=BOX, n_threads=8, max_iter=2_000_000, weight_pos=w[1], weight_neg=w[-1], **KERNELS[name])
    rows, mn, mx = _rows(X)
    K = D.kfun_block(rows, rows, p).cpu().numpy()  # the device's own kernel values
    pts = 2 * n if est == "svr" else n
    alpha = torch.empty(pts, dtype=torch.float64, device=DEV)
    dt = N.DecompTrace(400, pts)
    if est == "svr":
        res, _ = D.train_decomp_svr(rows, torch.from_numpy(z).to(DEV), alpha, p, mn, mx, epsilon=EPSILON,
                                    working_set=q, trace=dt)
        a_o, r_o, _, ot = C.decomp_train_gram_svr(K, z, p, EPSILON, q=q, inner_wss=2, trace_cap=400, snapshots=True)
    else:
        res, _ = D.train_decomp(rows, torch.from_numpy(y).to(DEV), alpha, p, mn, mx, working_set=q, trace=dt)
        a_o, r_o, _, ot = C.decomp_train_gram(K, y, p, q=q, inner_wss=2, trace_cap=400, snapshots=True)
    _compare(dt, ot)
    a = alpha.cpu().numpy()
    np.testing.assert_array_equal(a, a_o)
    assert res.stop_reason == r_o.stop_reason == "converged" and res.b == r_o.b and res.iterations == r_o.iterations
    # the KKT gap on all points from an independent float64 Gram and the returned alpha
    Kn = C.kernel_gram(X, X, p)
    if est == "svr":
        s = np.r_[np.ones(n), -np.ones(n)]
        f = np.tile(Kn @ (a[:n] - a[n:]), 2) + np.r_[EPSILON - z, -EPSILON - z]
        box = np.full(2 * n, p.C)
    else:
        s, f, box = y, Kn @ (a * y) - y, p.box(y)
    hi = ((s == 1) & (a < box - p.eps)) | ((s == -1) & (a > p.eps))
    lo = ((s == 1) & (a > p.eps)) | ((s == -1) & (a < box - p.eps))
    gap = f[lo].max() - f[hi].min()
    print(f"{name} {est} n={n} q={q}: outer {dt.count} gap {gap:.3e}")
    assert gap <= 2 * p.tau


@pytest.mark.parametrize("name", list(KERNELS))
def test_estimators_predict_and_match_the_fixture(name):
    fx = load_fixture()
    Xq = rows_labels_targets(50, 99)[0]
    for m, ref in ((SVC(C=BOX, tol=1e-6, device="cuda:0", **KERNELS[name]).fit(fx["X"], fx["y"]), fx[f"svc_{name}"]),
                   (SVR(C=BOX, tol=1e-6, epsilon=EPSILON, device="cuda:0", **KERNELS[name]).fit(fx["X"], fx["z"]),
                    fx[f"svr_{name}"])):
        assert m.stop_reason_ == "converged" and m.timings_["gram_path"] == "fp64"
        dec = m.decision_function if isinstance(m, SVC) else m.predict
        assert np.abs(dec(fx["X"]) - ref).max() <= FIXTURE_TOL[name]
        sv, coef = m.support_vectors_, m.dual_coef_
        kw = {"gamma": 1.0, **KERNELS[name]}
        Kq, kb = kernel_ref(Xq, sv, **kw)
        cnt, d = len(coef), Xq.shape[1]
        want = Kq.astype(np.longdouble) @ coef - m.b_  # the reference's own sum in longdouble
        bound = ((cnt + d + 4) * U * np.abs(Kq * coef).sum(1)
                 + (kb + (4 * TANH_DEV if name == "sigmoid" else 0)) @ np.abs(coef))
        err = np.abs(dec(Xq) - want).astype(np.float64)
        print(f"{name} {type(m).__name__}: max (err - bound) {(err - bound).max():.3e}, max err {err.max():.3e}")
        assert np.all(err <= bound)
        # a model padded past 1,024 support vectors with zero coefficients: two chunks, the same bits
        dv = m._dev
        pad = 1100 - cnt
        Xs = torch.cat([dv["Xs"], dv["Xs"][:1].expand(pad, -1)]).contiguous()
        cf = torch.cat([dv["coef"], torch.zeros(pad, dtype=torch.float64, device=DEV)])
        Xqd = m._device_queries(Xq)[0]
        one = D.decision_kfun(dv["Xs"], dv["coef"], Xqd, m.params, m.b_)
        assert torch.equal(D.decision_kfun(Xs, cf, Xqd, m.params, m.b_), one)


def _native_fit(kind, p, warm=False):
    X, y, z = rows_labels_targets(64, 5)
    rows, mn, mx = _rows(X)
    a = torch.zeros(128, dtype=torch.float64, device=DEV)
    yd, zd = torch.from_numpy(y).to(DEV), torch.from_numpy(z).to(DEV)
    if kind == "svc":
        return D.train_decomp(rows, yd, a[:64], p, mn, mx, warm=warm)
    if kind == "svr":
        return D.train_decomp_svr(rows, zd, a, p, mn, mx)
    if kind == "csr":
        sp = pytest.importorskip("scipy.sparse")
        A = D.upload_csr(sp.csr_matrix(X), DEV)
        D.csr_prepare(A)
        return D.train_decomp_csr(A, a[:64], p, y=yd)
    if kind == "heldout":
        return D.train_decomp_heldout(rows, yd, torch.zeros(64, dtype=torch.uint8, device=DEV), a[:64], a[64:], p, mn, mx)
    if kind == "oneclass":
        return D.train_decomp_oneclass(rows, a[:64], p, mn, mx)
    if kind == "nusvc":
        return D.train_decomp_nusvc(rows, yd, a[:64], p, mn, mx, nu=0.3)
    return D.train_decomp_nusvr(rows, zd, a, p, mn, mx, nu=0.3)


@pytest.mark.parametrize("kind,env,kw,msg", [
    ("svc", {"SVM355_DECOMP_WSS": "3"}, {}, "does not support SVM355_DECOMP_WSS other than 2"),
    ("svr", {"SVM355_DECOMP_NT": "128"}, {}, "does not support SVM355_DECOMP_NT other than 256"),
    ("svc", {"SVM355_DECOMP_CCACHE": "1"}, {}, "does not support a forced column cache"),
    ("svc", {"SVM355_DECOMP_NEWTON": "1"}, {}, "poly kernel does not support the Newton polish"),
    ("svc", {}, {"shrinking": True}, "poly kernel does not support shrinking"),
    ("svc", {}, {"warm": True}, "poly kernel does not support a warm start"),
    ("csr", {}, {}, "poly kernel does not support sparse"),
    ("heldout", {}, {}, "poly kernel does not support this mode"),
    ("oneclass", {}, {}, "poly kernel does not support this mode"),
    ("nusvc", {}, {}, "poly kernel does not support this mode"),
    ("nusvr", {}, {}, "poly kernel does not support this mode")])
def test_the_solver_refuses_what_a_dot_kernel_does_not_cover(kind, env, kw, msg, monkeypatch):
    """The native refusal table and knob check (decomp_mode.h, decomp.hip) through the C entries: a ValueError
    with the table's message.  (world > 1 shares the table: tests/test_kfun_cpu.py reaches it on the CPU oracle.)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    warm = kw.pop("warm", False)
    with pytest.raises(ValueError, match=msg):
        _native_fit(kind, SVMParams(kernel="poly", **kw), warm=warm)


@pytest.mark.parametrize("kw,msg", [
    ({"solver": "smo"}, "solver='smo'"), ({"wss": "second"}, "wss='second'"), ({"gram": "fp64"}, "gram='fp64'"),
    ({"kcache": "rows"}, "kcache='rows'"), ({"scale": False}, "scale=False"), ({"probability": True}, "probability"),
    ({"shrinking": True}, "does not support shrinking"), ({"alpha0": True}, "does not support a warm start"),
    ({"sparse": True}, "sparse rows")])
def test_the_estimator_refuses_with_a_value_error(kw, msg):
    X, y, _ = rows_labels_targets(64, 5)
    fit = {"alpha0": np.zeros(64)} if kw.pop("alpha0", False) else {}
    if kw.pop("sparse", False):
        X = pytest.importorskip("scipy.sparse").csr_matrix(X)
    with pytest.raises(ValueError, match=msg):
        SVC(device="cuda:0", kernel="poly", **kw).fit(X, y, **fit)
