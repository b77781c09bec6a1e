"""Class weights on the GPU: the decomposition solver's weighted selection kernels and weighted inner solve
(ws_inner_kernel's CW variants) against their CPU oracle bit for bit, against an independent FP64 kernel,
and through the estimators and the CLI.

Data: synthetic_mnist(n, seed=77), digit 1 against the rest; C = 10, gamma = 0.00125, tau = 1e-5; weight
pairs A = (pos 2.0, neg 0.5) and B = (pos 0.5, neg 2.0), which give bounded and free support vectors in both
classes (asserted per solution), so both branches of the pair clip run with two different boxes."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from svm355 import SVC, OneVsRestSVC, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C
from svm355.ops import device as D
from svm355.utils.data import synthetic_mnist

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = Path(__file__).resolve().parents[1]
PAIRS = {"A": (2.0, 0.5), "B": (0.5, 2.0)}
CW_A = {1: 2.0, -1: 0.5}


def _params(w, **kw):
    return SVMParams(weight_pos=w[0], weight_neg=w[1], **kw)


# ---- helpers of test_gpu_decomp_oracle.py (copied: existing test files stay as they are) ------------------
def _dev_rows(tr):
    Xu = D.upload_u8(tr.X, DEV)
    mmd = torch.empty(2 * tr.d, dtype=torch.float64, device=DEV)
    mn, mx = D.minmax_u8(Xu, out=mmd)
    mm = mmd.cpu().numpy()
    return Xu, mm[: tr.d].copy(), mm[tr.d:].copy()


def _exact_gram_host(Xu, mn, mx, n):
    K = D.rbf_gram_u8(Xu, 0.00125, mn, mx)
    assert K is not None
    out = K[:n, :n].cpu().numpy()
    del K
    D.release_gram_buffers()
    torch.cuda.empty_cache()
    return np.ascontiguousarray(out)


def _compare(dt, ot):
    dr, orr = dt.records(), ot.records()
    assert len(dr) == len(orr) and len(dr) > 0
    for o, (a, b) in enumerate(zip(dr, orr)):
        assert a["m"] == b["m"], o
        np.testing.assert_array_equal(a["W"], b["W"], err_msg=f"outer {o}: working set")
        assert a["inner"] == b["inner"], o
        np.testing.assert_array_equal(a["bounds"], b["bounds"], err_msg=f"outer {o}: bounds")
        np.testing.assert_array_equal(a["cols"], b["cols"], err_msg=f"outer {o}: moved columns")
        np.testing.assert_array_equal(a["coef"], b["coef"], err_msg=f"outer {o}: coefficients")
        np.testing.assert_array_equal(a["alpha"], b["alpha"], err_msg=f"outer {o}: alpha")
        np.testing.assert_array_equal(a["f"], b["f"], err_msg=f"outer {o}: f")


@pytest.fixture(scope="module")
def prob2k():
    """n = 2000: the rows on the device, their statistics, and the device's own exact Gram on the host."""
    tr = synthetic_mnist(2000, seed=77).compact()
    assert tr.X.dtype == np.uint8
    Xu, mn, mx = _dev_rows(tr)
    K = _exact_gram_host(Xu, mn, mx, 2000)
    return tr, Xu, mn, mx, K


def has_bounded_and_free_in_both_classes(y, a, p):
    box = p.box(y)
    bounded = a >= box * (1 - 1e-9)
    free = (a > p.sv_tol) & ~bounded
    counts = {(s, k): int((m & (y == s)).sum()) for s in (1, -1) for k, m in (("bounded", bounded), ("free", free))}
    assert all(v >= 1 for v in counts.values()), f"the solution no longer exercises both clips: {counts}"


def weighted_kkt_gap_fp64(X, y, a, p, scale=True):
    """decomp_checks.kkt_gap_fp64 over the WEIGHTED sets: b_low - b_high over all points from an independent
    FP64 RBF (torch), on the min-max scaled rows."""
    Xs = torch.from_numpy(np.asarray(X, dtype=np.float64)).to(DEV)
    if scale:
        mn, mx = Xs.min(0).values, Xs.max(0).values
        rng = torch.where(mx - mn < 1e-12, torch.ones_like(mx), mx - mn)
        Xs = (Xs - mn) / rng
    sq = (Xs * Xs).sum(1)
    ay = torch.from_numpy(a * y).to(DEV)
    Kb = torch.exp(-p.gamma * torch.clamp(sq[:, None] + sq[None, :] - 2.0 * (Xs @ Xs.T), min=0.0))
    f = (Kb @ ay).cpu().numpy() - y
    box = p.box(y)
    hi = ((y == 1) & (a < box - p.eps)) | ((y == -1) & (a > p.eps))
    lo = ((y == 1) & (a > p.eps)) | ((y == -1) & (a < box - p.eps))
    return f[lo].max() - f[hi].min()


def kkt_checks(X, y, a, p):
    gap = weighted_kkt_gap_fp64(X, y, a, p)
    box = p.box(y)
    print(f"weighted KKT gap {gap:.3e} (bound {2 * p.tau + 1e-9:.3e}), max alpha {a.max():.6g}")
    assert gap <= 2 * p.tau + 1e-9
    assert np.all(a >= -1e-9 * box) and np.all(a <= box * (1 + 1e-9))
    assert abs(np.dot(a, y)) <= 1e-9 * max(1.0, a.sum())
    assert np.any(a > p.C), "no alpha above C: the weights did not take effect"


# ---- 1. the device trajectory is the CPU oracle's under weights ------------------------------------------
@pytest.mark.parametrize("wss", [3, 1, 2])
@pytest.mark.parametrize("q", [64, 1024])
@pytest.mark.parametrize("pair", ["A", "B"])
def test_weighted_device_trajectory_equals_the_cpu_oracle(prob2k, pair, q, wss, monkeypatch):
    monkeypatch.setenv("SVM355_DECOMP_WSS", str(wss))
    tr, Xu, mn, mx, K = prob2k
    n = len(tr.y)
    p = _params(PAIRS[pair])
    yd = torch.from_numpy(tr.y).to(DEV)
    alpha = torch.empty(n, dtype=torch.float64, device=DEV)
    dt = N.DecompTrace(600, n)
    res, tm = D.train_decomp(Xu, yd, alpha, p, mn, mx, working_set=q, trace=dt)
    a_o, r_o, st_o, ot = C.decomp_train_gram(K, tr.y, _params(PAIRS[pair], n_threads=8), q=q, inner_wss=wss,
                                             trace_cap=600, snapshots=True)
    _compare(dt, ot)
    assert res.stop_reason == r_o.stop_reason == "converged"
    assert res.iterations == r_o.iterations and res.b == r_o.b
    a = alpha.cpu().numpy()
    np.testing.assert_array_equal(a, a_o)
    assert tm["outer_iterations"] == st_o["outer_iterations"] and tm["working_set"] == st_o["working_set"]
    has_bounded_and_free_in_both_classes(tr.y, a, p)
    assert a.max() > p.C


# ---- 2. warm start under weights -------------------------------------------------------------------------
def test_weighted_warm_start_equals_the_oracle_and_meets_the_stop_test(prob2k):
    tr, Xu, mn, mx, K = prob2k
    n = len(tr.y)
    p = _params(PAIRS["A"])
    half = tr.subset(0, n // 2)
    a_half = SVC(device="cuda:0", solver="decomp", class_weight=CW_A).fit(half.X, half.y).alpha_
    assert a_half.max() > p.C
    a0 = np.concatenate([a_half, np.zeros(n - n // 2)])
    yd = torch.from_numpy(tr.y).to(DEV)
    alpha = torch.from_numpy(a0.copy()).to(DEV)
    dt = N.DecompTrace(600, n)
    res, tm = D.train_decomp(Xu, yd, alpha, p, mn, mx, warm=True, trace=dt)
    a_o, r_o, _, ot = C.decomp_train_gram(K, tr.y, _params(PAIRS["A"], n_threads=8), alpha=a0, trace_cap=600,
                                          snapshots=True)
    _compare(dt, ot)
    a = alpha.cpu().numpy()
    np.testing.assert_array_equal(a, a_o)
    assert res.stop_reason == "converged" and res.b == r_o.b and tm["warm_start"]
    y = tr.y.astype(np.float64)
    f = K @ (a * y) - y
    box = p.box(tr.y)
    hi = ((y == 1) & (a < box - p.eps)) | ((y == -1) & (a > p.eps))
    lo = ((y == 1) & (a > p.eps)) | ((y == -1) & (a < box - p.eps))
    assert f[lo].max() - f[hi].min() <= 2 * p.tau + 1e-9
    warm = SVC(device="cuda:0", solver="decomp", class_weight=CW_A).fit(tr.X, tr.y, alpha0=a0)
    np.testing.assert_array_equal(warm.alpha_, a)


# ---- 3. the stop test from an independent kernel ---------------------------------------------------------
@pytest.fixture(scope="module")
def fit_A(prob2k):
    tr = prob2k[0]
    return SVC(device="cuda:0", class_weight=CW_A).fit(tr.X, tr.y)


def test_weighted_fit_meets_the_stop_test_of_an_independent_kernel(prob2k, fit_A):
    tr = prob2k[0]
    g = fit_A
    assert g.stop_reason_ == "converged" and g.timings_["solver"] == "decomp" and g.timings_["rows"] == "uint8"
    assert g.class_weight_ == CW_A
    has_bounded_and_free_in_both_classes(tr.y, g.alpha_, g.params)
    kkt_checks(tr.X, tr.y, g.alpha_, g.params)


# ---- 4. equal weights are the unweighted bits ------------------------------------------------------------
def test_equal_weights_are_the_unweighted_bits_on_the_device(prob2k):
    tr = prob2k[0]
    u = SVC(device="cuda:0").fit(tr.X, tr.y)
    w = SVC(device="cuda:0", class_weight={1: 1.0, -1: 1.0}).fit(tr.X, tr.y)
    assert np.array_equal(w.alpha_, u.alpha_) and w.b_ == u.b_ and w.n_iter_ == u.n_iter_
    assert np.array_equal(w.support_, u.support_) and len(u.support_) > 10


# ---- 5. input forms agree --------------------------------------------------------------------------------
def test_uint8_and_float64_rows_agree_under_weights(prob2k, fit_A):
    tr = prob2k[0]
    f64 = SVC(device="cuda:0", class_weight=CW_A).fit(tr.X.astype(np.float64), tr.y)
    assert f64.timings_["rows"] == "fp64" and f64.timings_["gram_path"] == "int8-exact"
    assert np.array_equal(f64.alpha_, fit_A.alpha_) and f64.b_ == fit_A.b_


# ---- 6. real-valued rows: the FP64-MFMA kernel values ----------------------------------------------------
def gaussian_rows():
    """Two overlapping Gaussian classes at 1:4, n = 1500, d = 20 (seeded).  The overlap (means +-0.35 per
    coordinate, unit variance) was chosen on the CPU oracle: under weights A at gamma = 0.125 its solution
    has bounded and free support vectors in both classes."""
    rng = np.random.default_rng(20261)
    n, d, n_pos = 1500, 20, 300
    y = -np.ones(n, dtype=np.int32)
    y[rng.choice(n, size=n_pos, replace=False)] = 1
    X = rng.standard_normal((n, d)) + 0.35 * y[:, None]
    return X, y


def test_real_valued_rows_under_weights():
    X, y = gaussian_rows()
    c = SVC(device="cpu", gamma=0.125, class_weight=CW_A).fit(X, y)
    has_bounded_and_free_in_both_classes(y, c.alpha_, c.params)
    g = SVC(device="cuda:0", gamma=0.125, class_weight=CW_A).fit(X, y)
    assert g.stop_reason_ == "converged" and g.timings_["solver"] == "decomp" and g.timings_["gram_path"] == "fp64"
    has_bounded_and_free_in_both_classes(y, g.alpha_, g.params)
    kkt_checks(X, y, g.alpha_, g.params)
    Xs = c.scaler_.transform(X)
    sq = np.einsum("ij,ij->i", Xs, Xs)
    K = np.exp(-0.125 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * Xs @ Xs.T, 0.0))

    def objective(a):
        ay = a * y
        return a.sum() - 0.5 * ay @ (K @ ay)

    og, oc = objective(g.alpha_), objective(c.alpha_)
    print(f"objective device {og:.12f} cpu {oc:.12f} rel {abs(og - oc) / abs(oc):.3e}")
    assert abs(og - oc) <= 1e-8 * abs(oc)


# ---- 7. one-vs-rest --------------------------------------------------------------------------------------
def test_one_vs_rest_balanced_equals_per_class_svc():
    ds = synthetic_mnist(1500, seed=77).compact()
    m = OneVsRestSVC(class_weight="balanced", device="cuda:0").fit(ds.X, ds.labels, classes=[0, 1, 2])
    assert m.timings_["smo_solver"] == "decomp"
    for k, c in enumerate(m.classes_):
        y = np.where(ds.labels == c, 1, -1).astype(np.int32)
        s = SVC(class_weight="balanced", device="cuda:0").fit(ds.X, y)
        assert m.class_weight_[k] == s.class_weight_ and s.class_weight_[1] > 1.0 > s.class_weight_[-1]
        assert np.array_equal(m.dual_coef_[:, k], (s.alpha_ * y)[m.support_]), f"class {c}"
        assert set(s.support_) <= set(m.support_)
        assert m.intercepts_b_[k] == s.b_
        assert s.alpha_.max() > s.params.C


# ---- 8. what is not built, or unweighted, refuses --------------------------------------------------------
@pytest.mark.parametrize("env,msg", [
    ({"SVM355_DECOMP_NEWTON": "1"}, "class weights are not supported with the Newton polish"),
    ({"SVM355_DECOMP_NT": "128"}, "the weighted inner solve is not built for SVM355_DECOMP_NT=128 SVM355_DECOMP_WSS=3"),
    ({"SVM355_DECOMP_NT": "64"}, "the weighted inner solve is not built for SVM355_DECOMP_NT=64"),
    ({"SVM355_DECOMP_NT": "512"}, "the weighted inner solve is not built for SVM355_DECOMP_NT=512"),
    ({"SVM355_DECOMP_WSS": "4"}, "the weighted inner solve is not built for SVM355_DECOMP_NT=256 SVM355_DECOMP_WSS=4"),
    ({"SVM355_DECOMP_PROF": "1"}, "SVM355_DECOMP_PROF=1"),
], ids=lambda v: "-".join(f"{k[14:]}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_unbuilt_weighted_variants_refuse(prob2k, monkeypatch, env, msg):
    tr = prob2k[0]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(N.NativeError) as e:
        SVC(device="cuda:0", class_weight=CW_A).fit(tr.X, tr.y)
    assert msg in str(e.value)
    for k in env:
        monkeypatch.delenv(k)
    g = SVC(device="cuda:0", class_weight=CW_A).fit(tr.X, tr.y)  # and the device is fine afterwards
    assert g.stop_reason_ == "converged"


def test_shrinking_and_the_pairwise_entries_refuse_natively(prob2k):
    tr, Xu, mn, mx, K = prob2k
    n = len(tr.y)
    yd = torch.from_numpy(tr.y).to(DEV)
    alpha = torch.zeros(n, dtype=torch.float64, device=DEV)
    with pytest.raises(N.NativeError, match="class weights are not supported with shrinking"):
        D.train_decomp(Xu, yd, alpha, _params(PAIRS["A"], shrinking=True), mn, mx)
    Kd = torch.from_numpy(K).to(DEV)
    with pytest.raises(N.NativeError, match="svmd_smo: class weights"):
        D.smo(Kd, yd, alpha, _params(PAIRS["A"]))
    with pytest.raises(N.NativeError, match="svmd_train_u8: class weights"):
        D.train_u8(Xu, yd, alpha, _params(PAIRS["A"]), mn, mx)
    with pytest.raises(N.NativeError, match="class weights must be finite and > 0"):
        _bad_weight_fit(Xu, yd, alpha, mn, mx)


def _bad_weight_fit(Xu, yd, alpha, mn, mx):
    """svmd_train_decomp with a negative weight in the struct (SVMParams itself refuses to hold one)."""
    import ctypes

    ctx = D._ctx_for(Xu)
    a, b, _ = D._host_stats(mn, mx)
    p = N.params_struct(weight_pos=-1.0)
    r, tm, used = N.SvmResult(), N.SvmdTiming(), ctypes.c_int32(0)
    N.check(ctx.lib.svmd_train_decomp(ctx.bind(), N.ptr(Xu), 1, Xu.shape[0], Xu.shape[1], Xu.shape[1], N.ptr(a), N.ptr(b),
                                      N.ptr(yd), N.ptr(alpha), ctypes.byref(p), 1024, 0, ctypes.byref(r),
                                      ctypes.byref(tm), None, ctypes.byref(used), None), "svmd_train_decomp")


# ---- 9. the CLI ------------------------------------------------------------------------------------------
def test_gpu_cli_honours_the_weights(prob2k, fit_A, tmp_path):
    exe = ROOT / "svm355" / "bin" / "svm_gpu"
    out = tmp_path / "gpu.json"
    base = [str(exe), "--synthetic", "2000,500", "--seed", "77", "--weight-pos", "2", "--weight-neg", "0.5", "--quiet"]
    r = subprocess.run(base + ["--json", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    j = json.loads(out.read_text())
    assert j["weight_pos"] == 2.0 and j["weight_neg"] == 0.5 and j["solver"] == "decomp"
    assert j["n_sv"] == len(fit_A.support_) and j["b"] == fit_A.b_
    r = subprocess.run(base + ["--solver", "smo"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--weight-pos / --weight-neg need the decomposition solver" in r.stderr
