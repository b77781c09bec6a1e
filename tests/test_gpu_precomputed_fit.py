"""SVC / SVR with kernel="precomputed" on the GPU decomposition solver: the device trajectory against the CPU oracle on
the same Gram (bit for bit), the scikit-learn fixture through the linear Gram, prediction, save / load, refusals."""
import numpy as np
import pytest
import torch

from svm355 import CSR, SVC, SVR, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C
from svm355.ops import device as D

from kfun_checks import C as BOX, EPSILON, FIXTURE_TOL, U, load_fixture
from test_gpu_decomp_oracle import _compare
from test_precomputed_cpu import grams

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    f = load_fixture()
    return f, grams(f["X"])


@pytest.mark.parametrize("est", ["svc", "svc_weighted", "svr"])
@pytest.mark.parametrize("name,q", [("linear", 1024), ("linear", 64), ("rbf", 256)])
def test_trajectory_equals_the_oracle_bit_for_bit(fx, name, q, est):
    f, G = fx
    K, y, z = G[name], f["y"], f["z"]
    n = len(y)
    w = (2.0, 0.5) if est == "svc_weighted" else (1.0, 1.0)
    p = SVMParams(C=BOX, n_threads=8, max_iter=2_000_000, weight_pos=w[0], weight_neg=w[1], kernel="precomputed")
    Kd = D.device_gram(K, DEV)
    assert D.gram_check(Kd) == -1
    pts = 2 * n if est == "svr" else n
    alpha = torch.empty(pts, dtype=torch.float64, device=DEV)
    dt = N.DecompTrace(400, pts)
    if est == "svr":
        res, tm = D.train_decomp_gram(Kd, alpha, p, z=torch.from_numpy(z).to(DEV), epsilon=EPSILON, working_set=q, trace=dt)
        a_o, r_o, _, ot = C.decomp_train_gram_svr(K, z, p, EPSILON, q=q, inner_wss=2, trace_cap=400, snapshots=True)
    else:
        res, tm = D.train_decomp_gram(Kd, alpha, p, y=torch.from_numpy(y).to(DEV), working_set=q, trace=dt)
        a_o, r_o, _, ot = C.decomp_train_gram(K, y, p, q=q, inner_wss=2, trace_cap=400, snapshots=True)
    _compare(dt, ot)
    np.testing.assert_array_equal(alpha.cpu().numpy(), a_o)
    assert res.stop_reason == r_o.stop_reason == "converged" and res.b == r_o.b and res.iterations == r_o.iterations
    assert tm["gram_path"] == "precomputed"


def test_estimators_match_the_fixture_predict_and_round_trip(fx, tmp_path):
    f, G = fx
    K = G["linear"]  # the fixture's rows are their own min-max scaling
    Kq = np.ascontiguousarray(K[:50] * 1.25)  # any (m, n) query Gram
    for cls, m, ref in ((SVC, SVC(C=BOX, tol=1e-6, device="cuda:0", kernel="precomputed").fit(K, f["y"]), f["svc_linear"]),
                        (SVR, SVR(C=BOX, tol=1e-6, epsilon=EPSILON, device="cuda:0", kernel="precomputed").fit(K, f["z"]),
                         f["svr_linear"])):
        assert m.stop_reason_ == "converged" and m.scaler_ is None and m.support_vectors_.shape == (0, 0)
        dec = m.decision_function if cls is SVC else m.predict
        dev = np.abs(dec(K) - ref).max()
        print(f"{cls.__name__}: max |decision - fixture| {dev:.3e} (bound {FIXTURE_TOL['linear']:.3e})")
        assert dev <= FIXTURE_TOL["linear"]
        P = Kq[:, m.support_] * m.dual_coef_
        want = P.astype(np.longdouble).sum(1) - m.b_
        got = dec(Kq)
        err = np.abs(got - want).astype(np.float64)
        bound = (len(m.support_) / 64 + 8) * U * np.abs(P).sum(1)
        print(f"{cls.__name__}: {len(m.support_)} support columns, max err / bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound)
        np.testing.assert_array_equal(dec(torch.from_numpy(Kq).to(DEV)), got)  # a device tensor, in place
        m.save(tmp_path / cls.__name__)
        back = cls.load(tmp_path / cls.__name__, device="cuda:0")
        assert back.n_fit_ == K.shape[0] and back._dev is not None
        np.testing.assert_array_equal((back.decision_function if cls is SVC else back.predict)(Kq), got)
    # a Gram already on the device: used in place (even stride) or copied once (odd n), the same fit; the estimator's
    # device without an index ("cuda", and the default "auto") takes the tensor on the current device
    a = SVC(C=BOX, device="cuda:0", kernel="precomputed").fit(K, f["y"])
    b = SVC(C=BOX, device="cuda", kernel="precomputed").fit(torch.from_numpy(K).to(DEV), f["y"])
    r = SVR(C=BOX, kernel="precomputed").fit(torch.from_numpy(K).to(DEV), f["z"])
    assert r.stop_reason_ == "converged" and r.predict(torch.from_numpy(Kq).to(DEV)).shape == (50,)
    c = SVC(C=BOX, device="cuda:0", kernel="precomputed").fit(torch.from_numpy(K[:299, :299].copy()).to(DEV), f["y"][:299])
    np.testing.assert_array_equal(a.dual_coef_, b.dual_coef_)
    assert a.b_ == b.b_ and c.stop_reason_ == "converged"


def _asym(K):
    K = K.copy()
    K[3, 200] = np.nextafter(K[3, 200], np.inf)
    return K


@pytest.mark.parametrize("case,msg", [
    ("asymmetric", r"K\[3, 200\].*\(K \+ K\.T\) / 2"), ("not_square", "square"), ("query_width", r"X must be \(m, 300\)"),
    ("sample_weight", "sample_weight is not supported with kernel='precomputed'"),
    ("probability", "kernel='precomputed' is not supported with probability"), ("csr", "sparse"),
    ("float32", "row_dtype='float32' is not supported with kernel='precomputed'"),
    ("gram_dtype", "must be a float64 array"), ("query_dtype", "must be a float64 array")])
def test_the_estimator_refuses_with_a_value_error(fx, case, msg):
    f, G = fx
    K, y = G["linear"], f["y"]
    kw = {"probability": True} if case == "probability" else {"row_dtype": "float32"} if case == "float32" else {}
    m = SVC(C=BOX, device="cuda:0", kernel="precomputed", **kw)
    with pytest.raises(ValueError, match=msg):
        if case == "asymmetric":
            m.fit(_asym(K), y)
        elif case == "not_square":
            m.fit(K[:, :200], y)
        elif case == "query_width":
            m.fit(K, y).decision_function(K[:5, :200])
        elif case == "sample_weight":
            m.fit(K, y, sample_weight=np.ones(len(y)))
        elif case == "gram_dtype":
            m.fit(K.astype(np.float32), y)
        elif case == "query_dtype":
            m.fit(K, y).decision_function(K[:5].astype(np.float32))
        elif case == "csr":
            m.fit(CSR.from_dense(K), y)
        else:
            m.fit(K, y)


@pytest.mark.parametrize("kernel", ["precomputed", "laplacian"])
def test_the_dot_product_block_entries_refuse_any_other_kernel(kernel):
    rows = D.upload_rows(np.ones((4, 3)), DEV)
    coef = torch.ones(4, dtype=torch.float64, device=DEV)
    with pytest.raises(N.NativeError, match="a dot-product kernel"):
        D.kfun_block(rows, rows, SVMParams(kernel=kernel))
    with pytest.raises(N.NativeError, match="a dot-product kernel"):
        D.decision_kfun(rows, coef, rows, SVMParams(kernel=kernel), 0.0)
