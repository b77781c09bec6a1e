"""Sample weights on the GPU decomposition solver (decomp_box.hip): the device trajectory against the CPU oracle's
box arm bit for bit, the weighted dual's KKT conditions and the scikit-learn fixture for the estimators, a vector
of ones against the unweighted fit, and the refusals."""
import numpy as np
import pytest
import torch

from svm355 import SVC, SVR, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C
from svm355.ops import device as D

from sample_weight_checks import BOX, EPSILON, GAMMA, check_kkt, load_fixture, problem
from test_gpu_decomp_oracle import _compare

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _device_problem(X, gamma):
    """The device rows of X (uint8 bytes, or FP64 rows scaled there), their statistics and the device's own Gram."""
    n, d = X.shape
    if X.dtype == np.uint8:
        rows = D.upload_u8(X, DEV)
        mm = torch.empty(2 * d, dtype=torch.float64, device=DEV)
        D.minmax_u8(rows, out=mm)
        mn, mx = mm[:d].cpu().numpy().copy(), mm[d:].cpu().numpy().copy()
        K = D.rbf_gram_u8(rows, gamma, mn, mx)[:n, :n].cpu().numpy()
        D.release_gram_buffers()
    else:
        rows = D.upload_rows(X, DEV)
        mm = D.minmax_scale_(rows, d)
        mn, mx = mm[0].cpu().numpy(), mm[1].cpu().numpy()
        nrm = D.row_norms(rows, d)  # the solve's own norms
        Kq, path = D.rbf_gram_sym(rows, nrm, gamma, mn, mx)  # rows of integers (n = 2) admit the exact-integer plan
        if path == "fp64":
            Kq = D.rbf_gram(rows, nrm, rows, nrm, gamma, symmetric=True)
        K = Kq[:n, :n].cpu().numpy()
        del Kq
        D.release_gram_buffers()
    return rows, mn, mx, np.ascontiguousarray(K)


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp64"])
@pytest.mark.parametrize("n,q,twin", [(2, 1024, False), (300, 16, False), (4097, 64, False), (300, 32, True)])
def test_trajectory_equals_the_oracles_box_arm(n, q, twin, u8):
    X, _, y, z, w = problem(n, 10 + n, u8=u8)
    p = SVMParams(C=BOX, gamma=GAMMA, n_threads=8, weight_pos=1.0 if twin else 2.0, weight_neg=1.0 if twin else 0.5)
    rows, mn, mx, K = _device_problem(X, p.gamma)
    pts = 2 * n if twin else n
    alpha = torch.empty(pts, dtype=torch.float64, device=DEV)
    dt = N.DecompTrace(1500, pts)
    target = z if twin else y
    res, tm = D.train_decomp_sw(rows, torch.from_numpy(target).to(DEV), torch.from_numpy(w).to(DEV), alpha, p, mn, mx,
                                epsilon=EPSILON if twin else None, working_set=q, trace=dt)
    a_o, r_o, st_o, ot = C.decomp_train_gram_sw(K, target, w, p, epsilon=EPSILON if twin else None, q=q, inner_wss=2,
                                                trace_cap=1500, snapshots=True, fp64_rows=tm["gram_path"] == "fp64")
    print(f"n={n} q={q} twin={twin} rows={tm['rows']} path={tm['gram_path']}: outer {tm['outer_iterations']}, "
          f"pair updates {res.iterations - 1}")
    _compare(dt, ot)
    a = alpha.cpu().numpy()
    np.testing.assert_array_equal(a, a_o)
    assert res.stop_reason == r_o.stop_reason == "converged" and res.b == r_o.b and res.iterations == r_o.iterations
    assert tm["outer_iterations"] == st_o["outer_iterations"] and tm["inner_threads"] == 256
    assert np.all(a[np.tile(w, pts // n) == 0] == 0.0)


@pytest.fixture(scope="module")
def fixture_fits():
    fx = load_fixture()
    kw = dict(C=float(fx["C"]), gamma=float(fx["gamma"]), tol=float(fx["tol"]), device="cuda:0")
    return fx, kw, (SVC(**kw).fit(fx["X"], fx["y"], sample_weight=fx["w"]),
                    SVR(epsilon=float(fx["epsilon"]), **kw).fit(fx["X"], fx["z"], sample_weight=fx["w"]))


def test_estimators_meet_the_kkt_conditions_and_the_scikit_learn_fixture(fixture_fits):
    fx, _, (svc, svr) = fixture_fits
    for name, m, target, dec in (("svc", svc, fx["y"], svc.decision_function), ("svr", svr, fx["z"], svr.predict)):
        assert m.stop_reason_ == "converged" and m.timings_["solver"].endswith("-sw")
        check_kkt(m, fx["X"], target, fx["w"], m.params.tau)
        err = np.abs(dec(fx["Xte"]) - fx[f"{name}_ref"]).max()
        print(f"{name}: max |dec - sklearn(tol=1e-10)| = {err:.3e}, delta = {float(fx[name + '_delta']):.3e}")
        assert err <= 10 * float(fx[f"{name}_delta"])


def test_weights_of_one_give_the_unweighted_support_set(fixture_fits):
    fx, kw, _ = fixture_fits
    # the support set belongs to the optimum: the two pair sequences agree on it once the stop tolerance is below
    # what the least-determined support vector needs (at the fixture's 1e-3 a stop may leave one at zero)
    kw = {**kw, "tol": 1e-6}
    ones = SVC(**kw).fit(fx["X"], fx["y"], sample_weight=np.ones(len(fx["y"])))
    plain = SVC(**kw).fit(fx["X"], fx["y"])
    assert ones.timings_["solver"] == "decomp-sw" and plain.timings_["solver"] == "decomp"
    np.testing.assert_array_equal(ones.support_, plain.support_)
    assert np.abs(ones.decision_function(fx["Xte"]) - plain.decision_function(fx["Xte"])).max() <= 10 * float(fx["svc_delta"])


def _native_fit(kind, p, rows="u8"):
    X, _, y, z, w = problem(64, 5, u8=rows == "u8")
    r, mn, mx, _ = _device_problem(X, p.gamma)
    a = torch.zeros(128, dtype=torch.float64, device=DEV)
    wd = torch.from_numpy(w).to(DEV)
    if kind == "svr":
        return D.train_decomp_sw(r, torch.from_numpy(z).to(DEV), wd, a, p, mn, mx, epsilon=EPSILON)
    return D.train_decomp_sw(r, torch.from_numpy(y).to(DEV), wd, a[:64], p, mn, mx)


@pytest.mark.parametrize("kind,rows,env,kw,msg", [
    ("svc", "u8", {"SVM355_DECOMP_WSS": "3"}, {}, "SVM355_DECOMP_WSS other than 2"),
    ("svr", "u8", {"SVM355_DECOMP_NT": "128"}, {}, "SVM355_DECOMP_NT other than 256"),
    ("svc", "u8", {"SVM355_DECOMP_NEWTON": "1"}, {}, "the Newton polish"),
    ("svc", "u8", {}, {"shrinking": True}, "shrinking"),
    ("svr", "f64", {}, {"kernel": "poly"}, "a dot-product kernel")])
def test_the_solver_refuses_what_sample_weights_do_not_cover(kind, rows, env, kw, msg, monkeypatch):
    """The native refusal table and knob check (decomp_mode.h, decomp.hip) through the C entries."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(ValueError, match="sample weights do not support " + msg):
        _native_fit(kind, SVMParams(C=BOX, gamma=GAMMA, **kw), rows)


@pytest.mark.parametrize("kw,msg", [({"solver": "smo"}, "solver='smo' on a GPU"), ({"gram": "fp64"}, "gram='fp64'"),
                                    ({"kcache": "rows"}, "kcache='rows'"), ({"scale": False}, "scale=False on a GPU")])
def test_the_estimator_refuses_the_pairwise_gpu_solver(kw, msg):
    X, _, y, _, w = problem(64, 5)
    with pytest.raises(ValueError, match="sample_weight is not supported with " + msg):
        SVC(device="cuda:0", **kw).fit(X, y, sample_weight=w)
