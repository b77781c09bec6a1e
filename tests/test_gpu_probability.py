"""Platt probabilities and k-fold cross-validation on the GPU: the decomposition solver's held-out mode
(svmd_train_decomp_heldout: label 0 = held out, never selected; decomp.hip) against its CPU oracle bit for bit, the
one-workgroup sigmoid fit (svmd_platt_fit, platt.hip) at its wave, workgroup and residency edges, the GPU estimator
against scikit-learn's fixtures, the pooled folds against the same solves one after another, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

from svm355 import SVC, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C
from svm355.ops import device as D
from svm355.utils.data import synthetic_mnist

from decomp_mode_checks import check_refusal
from decomp_mode_checks import pixel_rows as mode_rows
from probability_checks import (FIXTURES, GRAD_TOL, block0_mask, check_fixture, load_fixture, platt_gradient,
                                proba_rows, synthetic_pairs)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PLATT_RESIDENT = 8192  # platt.hip: 1,024 threads x 8 pairs in registers; beyond it every pass streams


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


def _heldout_equals_oracle(Xdev, mn, mx, K, y, mask, p, q, fp64_rows, cap=1500):
    """One held-out solve on the device and on the oracle (given the device's own kernel values): the whole
    trajectory, alpha, b, the iteration counts and the held-out decisions, bit for bit."""
    n = K.shape[0]
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.int32)).to(DEV)
    md = torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    alpha = torch.full((n,), 7.0, dtype=torch.float64, device=DEV)  # the cold start overwrites it
    dec = torch.full((n,), 7.0, dtype=torch.float64, device=DEV)
    dt = N.DecompTrace(cap, n)
    out = D.train_decomp_heldout(Xdev, yd, md, alpha, dec, p, mn, mx, working_set=q, trace=dt)
    assert out is not None
    res, tm = out
    a_o, r_o, st_o, f_o, ot = C.decomp_train_gram_heldout(K, y, mask, p.replace(n_threads=8), q=q, trace_cap=cap,
                                                          snapshots=True, fp64_rows=fp64_rows)
    outers = _compare(dt, ot)
    assert res.stop_reason == r_o.stop_reason == "converged"
    assert res.iterations == r_o.iterations and res.b == r_o.b
    assert res.b_high == r_o.b_high and res.b_low == r_o.b_low
    assert tm["outer_iterations"] == st_o["outer_iterations"] == outers
    assert tm["inner_iterations"] == st_o["inner_iterations"] and tm["working_set"] == st_o["working_set"]
    a_d, dec_d = alpha.cpu().numpy(), dec.cpu().numpy()
    np.testing.assert_array_equal(a_d, a_o)
    assert np.all(a_d[mask] == 0.0)
    np.testing.assert_array_equal(dec_d[mask], f_o[mask] - r_o.b)
    assert np.all(dec_d[~mask] == 0.0)
    for rec in dt.records():
        assert not mask[rec["W"][: rec["m"]]].any()  # a held-out point is never selected
    return tm


@pytest.fixture(scope="module")
def pixel_rows():
    """2,000 uint8 pixel rows on the device, their bounds, and the device's own exact-integer kernel values."""
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
    return Xu, mn, mx, K, np.ascontiguousarray(tr.y, dtype=np.int32)


def _fp64_rows(X):
    """Real rows scaled on the device (the identity), and the device's own FP64 Gram on the host."""
    n = X.shape[0]
    Xd = D.upload_rows(X, DEV)
    mn, mx, _ = D.minmax_scale_(Xd, X.shape[1])
    nrm = D.row_norms(Xd, X.shape[1])  # the solve's own norms
    K = D.rbf_gram(Xd, nrm, Xd, nrm, 0.5, symmetric=True)[:n, :n].cpu().numpy()
    return Xd, mn.cpu().numpy(), mx.cpu().numpy(), np.ascontiguousarray(K)


@pytest.fixture(scope="module")
def real_rows_301():
    X, y, _ = proba_rows(301, 5)
    return _fp64_rows(X) + (y,)


# ---- the masked trajectory equals the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [None, (2.0, 0.5)])
def test_pixel_rows_with_a_whole_block_held_out(pixel_rows, weights):
    """n = 2,000, q = 64: 32 selection blocks of 63 rows, block 0 entirely held out (no candidate at all)."""
    Xu, mn, mx, K, y = pixel_rows
    p = SVMParams(C=10.0, gamma=0.00125, tau=1e-5, max_iter=10**7)
    if weights:
        p = p.replace(weight_pos=weights[0], weight_neg=weights[1])
    mask = block0_mask(2000)
    tm = _heldout_equals_oracle(Xu, mn, mx, K, y, mask, p, 64, fp64_rows=False)
    assert tm["gram_path"] == "int8-exact" and tm["outer_iterations"] >= 2 and tm["working_set"] == 64


@pytest.mark.parametrize("weights", [None, (2.0, 0.5)])
def test_fp64_rows_fold(real_rows_301, weights):
    Xd, mn, mx, K, y = real_rows_301
    p = SVMParams(C=10.0, gamma=0.5, tau=1e-5, max_iter=10**7)
    if weights:
        p = p.replace(weight_pos=weights[0], weight_neg=weights[1])
    mask = np.arange(301) % 5 == 2
    tm = _heldout_equals_oracle(Xd, mn, mx, K, y, mask, p, 64, fp64_rows=True)
    assert tm["gram_path"] == "fp64" and tm["outer_iterations"] >= 2


# ---- edges of the mask ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one_row", "last_n_mod_64_rows"])
def test_mask_edges(real_rows_301, case):
    Xd, mn, mx, K, y = real_rows_301
    mask = np.zeros(301, dtype=bool)
    if case == "one_row":
        mask[137] = True
    else:
        mask[301 - 301 % 64:] = True  # the last 45 rows
        assert mask.sum() == 45
    p = SVMParams(C=10.0, gamma=0.5, tau=1e-5, max_iter=10**7)
    _heldout_equals_oracle(Xd, mn, mx, K, y, mask, p, 64, fp64_rows=True)


def test_one_class_confined_to_one_block():
    """n = 2 x 63: the positives are rows 0..62, the negatives rows 63..125; every 4th row is held out."""
    X, y, _ = proba_rows(126, 8)
    o = np.argsort(-y, kind="stable")
    X, y = np.ascontiguousarray(X[o]), np.ascontiguousarray(y[o])
    assert np.all(y[:63] == 1) and np.all(y[63:] == -1)
    Xd, mn, mx, K = _fp64_rows(X)
    mask = np.arange(126) % 4 == 1
    p = SVMParams(C=10.0, gamma=0.5, tau=1e-5, max_iter=10**7)
    _heldout_equals_oracle(Xd, mn, mx, K, y, mask, p, 64, fp64_rows=True)


# ---- svmd_platt_fit -------------------------------------------------------------------------------------------------
def _platt(dec, y, use=None):
    dd = torch.from_numpy(np.ascontiguousarray(dec, dtype=np.float64)).to(DEV)
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.int32)).to(DEV)
    ud = None if use is None else torch.from_numpy(np.ascontiguousarray(use, dtype=np.uint8)).to(DEV)
    return D.platt_fit(dd, yd, ud)


# the wave (63 / 64 / 65), workgroup (1,023 / 1,024 / 1,025) and residency (8,192 / 8,193) edges; 20,000: ~20 pairs
# per thread streamed
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, PLATT_RESIDENT, PLATT_RESIDENT + 1, 20000])
def test_platt_fit_sizes(n):
    dec, y = synthetic_pairs(n, seed=n)
    r = _platt(dec, y)
    g1, g2 = platt_gradient(dec, y, r.A, r.B)
    print(f"n = {n}: A = {r.A:.6f}, B = {r.B:.6f}, {r.iterations} iterations, {r.status}, "
          f"gradient ({g1:.2e}, {g2:.2e})")
    # one pair is one class: nothing to fit, and the start (A = 0, B = the prior's logit) is the optimum itself
    assert r.status == ("degenerate" if n == 1 else "converged")
    assert np.isfinite(r.A) and np.isfinite(r.B)
    assert abs(g1) < GRAD_TOL and abs(g2) < GRAD_TOL
    r2 = _platt(dec, y)
    assert (r2.A, r2.B, r2.iterations, r2.status) == (r.A, r.B, r.iterations, r.status)  # the same bits


@pytest.mark.parametrize("n", [1025, PLATT_RESIDENT + 1])
def test_platt_fit_mask_equals_the_subset(n):
    dec, y = synthetic_pairs(n, seed=3)
    use = np.arange(n) % 3 != 1
    a = _platt(dec, y, use)
    g1, g2 = platt_gradient(dec, y, a.A, a.B, use=use)  # the gradient over the pairs that count, and only them
    assert a.status == "converged" and abs(g1) < GRAD_TOL and abs(g2) < GRAD_TOL

@pytest.mark.parametrize("n", [300, PLATT_RESIDENT + 1])
def test_platt_fit_degenerate_inputs_return_a_status(n):
    dec, y = synthetic_pairs(n, seed=1)
    npos, nneg = int((y > 0).sum()), int((y < 0).sum())
    for d, lab, prior in ((dec, np.ones(n, dtype=np.int32), (1.0, n + 1.0)),
                          (dec, -np.ones(n, dtype=np.int32), (n + 1.0, 1.0)),
                          (np.full(n, 0.7), y, (nneg + 1.0, npos + 1.0))):
        r = _platt(d, lab)
        assert r.status == "degenerate" and r.iterations == 0 and r.A == 0.0
        assert np.isfinite(r.B) and abs(r.B - np.log(prior[0] / prior[1])) <= 1e-14 * max(1.0, abs(r.B))


# ---- the estimator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", FIXTURES)
def test_gpu_estimator_agrees_with_the_scikit_learn_fixture(n, seed):
    g = load_fixture(n, seed)
    m = SVC(C=g["C"], gamma=g["gamma"], tol=1e-6, max_iter=10**7, device="cuda:0", probability=True)
    m.fit(g["X"], g["y"], folds=g["folds"])
    assert m.stop_reason_ == "converged" and m.platt_.status == "converged"
    assert m.timings_["gram_path"] == "fp64" and m.timings_["cv_ms"] > 0 and m.timings_["platt_ms"] > 0
    np.testing.assert_array_equal(m.scaler_.min_, 0.0)  # the fixture's rows: scaling is the identity
    np.testing.assert_array_equal(m.scaler_.max_, 1.0)
    check_fixture(m, g, seed)
    # the model beside the folds is the plain fit's
    plain = SVC(C=g["C"], gamma=g["gamma"], tol=1e-6, max_iter=10**7, device="cuda:0").fit(g["X"], g["y"])
    np.testing.assert_array_equal(m.alpha_, plain.alpha_)
    assert m.b_ == plain.b_
    pr = m.predict_proba(g["Xq"])
    np.testing.assert_allclose(pr.sum(1), 1.0, rtol=0, atol=4.5e-16)
    np.testing.assert_array_equal(m.predict(g["Xq"]), np.where(m.decision_function(g["Xq"]) > 0, 1, -1))


@pytest.fixture(scope="module")
def pixel_problem():
    tr = synthetic_mnist(2000, seed=17).compact()
    return tr.X, np.ascontiguousarray(tr.y, dtype=np.int32)


def test_pooled_folds_equal_the_solves_one_after_another(pixel_problem):
    X, y = pixel_problem
    est = SVC(device="cuda:0", class_weight="balanced")
    pooled = est.cross_val_decision(X, y, cv=5, seed=1)
    assert est.cv_timings_["concurrent_solves"] == 5
    serial = est.cross_val_decision(X, y, cv=5, seed=1, concurrent_solves=1)
    assert est.cv_timings_["concurrent_solves"] == 1
    np.testing.assert_array_equal(pooled, serial)
    assert np.all(pooled != 0.0)  # every row was held out once
    acc = est.cross_val_score(X, y, cv=5, seed=1)
    assert acc == np.mean(np.where(pooled > 0, 1, -1) == y) and acc > 0.9


def test_pixel_rows_estimator(pixel_problem, tmp_path):
    """uint8 pixel rows through the exact-integer plan: the model is the plain fit's, the held-out values are the
    cross-validation's own, and the sigmoid travels through save / load to a device model."""
    X, y = pixel_problem
    m = SVC(device="cuda:0", probability=True, cv=4, cv_seed=2).fit(X, y)
    assert m.timings_["gram_path"] == "int8-exact" and m.platt_.status == "converged" and m.probA_ < 0
    assert len(m.timings_["fold_ms"]) == 4 and m.timings_["concurrent_solves"] == 5
    plain = SVC(device="cuda:0").fit(X, y)
    np.testing.assert_array_equal(m.alpha_, plain.alpha_)
    assert m.b_ == plain.b_
    np.testing.assert_array_equal(m.cv_decision_, SVC(device="cuda:0").cross_val_decision(X, y, cv=4, seed=2))
    g1, g2 = platt_gradient(m.cv_decision_, y, m.probA_, m.probB_)
    assert abs(g1) < GRAD_TOL and abs(g2) < GRAD_TOL
    m.save(tmp_path / "m")
    back = SVC.load(tmp_path / "m", device="cuda:0")
    np.testing.assert_array_equal(back.predict_proba(X[:100]), m.predict_proba(X[:100]))


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_native_refusals_launch_nothing(real_rows_301, monkeypatch):
    Xd, mn, mx, K, y = real_rows_301
    yd = torch.from_numpy(y).to(DEV)
    md = torch.from_numpy((np.arange(301) % 5 == 0).astype(np.uint8)).to(DEV)
    alpha = torch.full((301,), 7.0, dtype=torch.float64, device=DEV)
    dec = torch.full((301,), 7.0, dtype=torch.float64, device=DEV)
    with pytest.raises(N.NativeError, match="shrinking"):
        D.train_decomp_heldout(Xd, yd, md, alpha, dec, SVMParams(gamma=0.5, shrinking=True), mn, mx)
    monkeypatch.setenv("SVM355_DECOMP_NEWTON", "1")
    with pytest.raises(N.NativeError, match="Newton"):
        D.train_decomp_heldout(Xd, yd, md, alpha, dec, SVMParams(gamma=0.5), mn, mx)
    monkeypatch.delenv("SVM355_DECOMP_NEWTON")
    ctx = D.DeviceContext.get(DEV)
    r, tm, used, st = N.SvmResult(), N.SvmdTiming(), ctypes.c_int32(0), (ctypes.c_int64 * 16)()
    p = SVMParams().to_struct()
    for bad in ("mask", "dec"):  # a missing mask or output buffer
        rc = ctx.lib.svmd_train_decomp_heldout(ctx.bind(), N.ptr(Xd), 0, 301, Xd.shape[1], 6, N.ptr(mn), N.ptr(mx),
                                               N.ptr(yd), None if bad == "mask" else N.ptr(md), N.ptr(alpha),
                                               None if bad == "dec" else N.ptr(dec), ctypes.byref(p), 64,
                                               ctypes.byref(r), ctypes.byref(tm), st, ctypes.byref(used), None)
        assert rc != 0 and used.value == 0
    torch.cuda.synchronize(DEV)
    assert torch.all(alpha == 7.0) and torch.all(dec == 7.0)  # nothing ran


def test_estimator_refusals_on_the_gpu():
    X, y, _ = proba_rows(80, 2)
    for kw, what in ((dict(solver="smo"), "solver='smo'"), (dict(scale=False), "scale=True"),
                     (dict(shrinking=True), "shrinking"), (dict(wss="second"), "wss='second'")):
        with pytest.raises(ValueError, match=what):
            SVC(device="cuda:0", probability=True, **kw).fit(X, y)
        with pytest.raises(ValueError, match=what):
            SVC(device="cuda:0", **kw).cross_val_decision(X, y)
    with pytest.raises(ValueError, match="warm start"):
        SVC(device="cuda:0", probability=True).fit(X, y, alpha0=np.zeros(80))
    with pytest.raises(ValueError, match="lacks a class"):
        SVC(device="cuda:0", probability=True).fit(X, y, folds=np.where(y == 1, 0, 1 + np.arange(80) % 3))
    with pytest.raises(ValueError, match="predict_proba needs"):
        SVC(device="cuda:0").fit(X, y).predict_proba(X)


@pytest.mark.parametrize("feature", ["shrinking", "newton"])  # class weights are allowed
def test_entry_refuses_under_its_name_and_enqueues_nothing(feature, monkeypatch):
    rows = mode_rows(DEV)
    mask = torch.from_numpy((np.arange(64) % 4 == 3).astype(np.uint8)).to(DEV)
    alpha = torch.empty(64, dtype=torch.float64, device=DEV)
    dec = torch.empty(64, dtype=torch.float64, device=DEV)
    check_refusal("svmd_train_decomp_heldout", "held-out", feature,
                  lambda p: D.train_decomp_heldout(rows[0], rows[3], mask, alpha, dec, p, rows[1], rows[2]), rows,
                  monkeypatch)
