"""SVC / SVR with the laplacian and chi2 kernels on the GPU decomposition solver (fit, prediction, fixture, refusals)."""
import numpy as np
import pytest
import torch

from svm355 import CSR, SVC, SVR, SVMParams
from svm355.models._device import host_kernel_decision
from svm355.ops import cpu as C
from svm355.ops import device as D

from dist_checks import DEC_TOL, KERNELS, U, kernel_ref, FIXTURE
from kfun_checks import C as BOX, EPSILON

pytestmark = pytest.mark.gpu
DEV, FX = torch.device("cuda:0"), dict(np.load(FIXTURE))


def _est(est, tol=1e-5, device="cuda:0", **kw):
    if est == "svr":
        return SVR(C=BOX, tol=tol, epsilon=EPSILON, device=device, **kw)
    return SVC(C=BOX, tol=tol, device=device, class_weight={1: 2.0, -1: 0.5} if est == "svc_weighted" else None, **kw)


def _dec(m, X):
    return m.predict(X) if isinstance(m, SVR) else m.decision_function(X)


@pytest.mark.parametrize("est", ["svc", "svc_weighted", "svr"])
@pytest.mark.parametrize("name", list(KERNELS))
def test_fit_is_optimal_and_predicts_as_the_cpu_estimator_and_scikit_learn(name, est, tmp_path, fx=FX):
    X, Xq, t = fx["X"], fx["Xq"], fx["z" if est == "svr" else "y"]
    m = _est(est, **KERNELS[name]).fit(X, t)
    assert m.stop_reason_ == "converged" and m.timings_["gram_path"] == "fp64"
    p, n = m.params, len(t)  # the KKT gap on all points from the host Gram and the returned alpha
    Kn = C.kernel_gram(X, X, p)
    if est == "svr":
        a, s = np.r_[m.alpha_, m.alpha_star_], np.r_[np.ones(n), -np.ones(n)]
        f, box = np.tile(Kn @ (m.alpha_ - m.alpha_star_), 2) + np.r_[EPSILON - t, -EPSILON - t], np.full(2 * n, p.C)
    else:
        a, s, f, box = m.alpha_, t, Kn @ (m.alpha_ * t) - t, p.box(t)
    hi = ((s == 1) & (a < box - p.eps)) | ((s == -1) & (a > p.eps))
    lo = ((s == 1) & (a > p.eps)) | ((s == -1) & (a < box - p.eps))
    assert f[lo].max() - f[hi].min() <= 2 * p.tau
    assert np.abs(_dec(m, Xq) - _dec(_est(est, device="cpu", **KERNELS[name]).fit(X, t), Xq)).max() <= DEC_TOL[name]
    if est != "svc_weighted":  # the scikit-learn fixture: tol = 1e-6 on both sides, the same measured margin
        m6 = _est(est, tol=1e-6, **KERNELS[name]).fit(X, t)
        assert np.abs(_dec(m6, Xq) - fx[f"{est}_{name}"]).max() <= DEC_TOL[name]
    # the device sum against the host evaluation of the same model, within the block test's sum bound over the SVs
    coef = m.dual_coef_
    Kq, kb = kernel_ref(Xq, m.support_vectors_, **KERNELS[name])
    host = host_kernel_decision(m, Xq, coef)
    assert np.all(np.abs(_dec(m, Xq) - host) <= (len(coef) + 4) * U * np.abs(Kq * coef).sum(1) + kb @ np.abs(coef))
    m.save(tmp_path)
    back = type(m).load(tmp_path)
    assert back.params.kernel == name
    np.testing.assert_allclose(_dec(back, Xq), host, rtol=0, atol=1e-12)


@pytest.mark.parametrize("kw,msg", [
    ({"probability": True}, "probability"), ({"cv": True}, "cross validation"), ({"wss": "second"}, "wss='second'"),
    ({"alpha0": True}, "does not support a warm start"), ({"shrinking": True}, "does not support shrinking"),
    ({"solver": "smo"}, "solver='smo'"), ({"gram": "fp64"}, "gram='fp64'"), ({"kcache": "rows"}, "kcache='rows'"),
    ({"sparse": True}, "sparse rows"), ({"sw": True}, "sample_weight is not supported with kernel="),
    ({"row_dtype": "float32"}, "row_dtype='float32' is not supported with kernel="),
    ({"native": "warm"}, "laplacian kernel does not support a warm start"),
    ({"native": "shrinking"}, "laplacian kernel does not support shrinking"),
    ({"native": "oneclass"}, "laplacian kernel does not support this mode"),
    ({"chi2_query": True}, "kernel='chi2' needs non-negative values: column 0 of the queries")])
def test_refusals_are_value_errors_and_leave_the_context_usable(kw, msg, fx=FX):
    X, y = fx["X"][:64], fx["y"][:64]
    kw = dict(kw)
    with pytest.raises(ValueError, match=msg):
        if kw.get("native"):
            what = kw["native"]
            rows = D.upload_rows(X, DEV)
            mn, mx = (v.cpu().numpy() for v in D.minmax_scale_(rows, X.shape[1])[:2])
            p, a = SVMParams(kernel="laplacian", shrinking=what == "shrinking"), torch.zeros(64, dtype=torch.float64, device=DEV)
            (D.train_decomp_oneclass(rows, a, p, mn, mx) if what == "oneclass" else
             D.train_decomp(rows, torch.from_numpy(y).to(DEV), a, p, mn, mx, warm=what == "warm"))
        elif kw.pop("chi2_query", False):
            SVC(device="cuda:0", **KERNELS["chi2"]).fit(X, y).decision_function(X[:4] - 2.0)
        elif kw.pop("cv", False):
            SVC(device="cuda:0", kernel="laplacian").cross_val_decision(X, y, cv=2)
        else:
            fit = {"alpha0": np.zeros(64)} if kw.pop("alpha0", False) else {}
            fit.update({"sample_weight": np.ones(64)} if kw.pop("sw", False) else {})
            Xf = CSR.from_dense(X) if kw.pop("sparse", False) else X  # the project's own CSR: no scipy
            SVC(device="cuda:0", kernel="laplacian", **kw).fit(Xf, y, **fit)
    rows = D.upload_rows(X, DEV)
    assert bool((D.dist_block(rows, rows, SVMParams(kernel="laplacian")).diagonal() == 1.0).all())
