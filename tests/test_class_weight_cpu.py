"""Class weights (per-class box constraints, LIBSVM's -wi / scikit-learn's class_weight) on the CPU: the two
oracles against scikit-learn's solution (a committed fixture, scripts/make_class_weight_golden.py) and
against the problem itself (an independent KKT check), the bit-identities that tie the weighted code to
the unweighted one, the option's validation, the refusals of everything unweighted, persistence and the
serial CLI.

Data: synthetic_mnist(n, seed=77), digit 1 against the rest; C = 10, gamma = 0.00125, tau = 1e-5; weight
pairs A = (pos 2.0, neg 0.5) and B = (pos 0.5, neg 2.0).  Each gives bounded and free support vectors in
both classes at n = 600 and n = 2000 (asserted per solution), so both branches of the pair clip run with
two different boxes."""
import ctypes
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from svm355 import SVC, OneVsRestSVC, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C
from svm355.ops.device import SMOResult
from svm355.utils.data import MinMaxScaler, check_warm_start, resolve_class_weight, synthetic_mnist

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "class_weight_n600_seed77.npz"
PAIRS = {"A": (2.0, 0.5), "B": (0.5, 2.0)}
TAU = 1e-5


def _params(w=None, **kw):
    kw.setdefault("n_threads", 4)
    if w is not None:
        kw.update(weight_pos=w[0], weight_neg=w[1])
    return SVMParams(**kw)


class Problem:
    def __init__(self, n):
        ds = synthetic_mnist(n, seed=77)
        self.raw, self.y = ds.X, ds.y.astype(np.int32)
        self.X = MinMaxScaler().fit_transform(ds.X)
        sq = np.einsum("ij,ij->i", self.X, self.X)
        self.K = np.exp(-0.00125 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * self.X @ self.X.T, 0.0))
        np.fill_diagonal(self.K, 1.0)


@pytest.fixture(scope="module")
def problems():
    return {600: Problem(600), 2000: Problem(2000)}


def objective(K, y, a):
    ay = a * y
    return a.sum() - 0.5 * ay @ (K @ ay)


def has_bounded_and_free_in_both_classes(y, a, p):
    box = p.box(y)
    bounded = a >= box * (1 - 1e-9)
    free = (a > p.sv_tol) & ~bounded
    counts = {(s, k): int((m & (y == s)).sum()) for s in (1, -1) for k, m in (("bounded", bounded), ("free", free))}
    assert all(v >= 1 for v in counts.values()), f"the solution no longer exercises both clips: {counts}"


def kkt_checks(K, y, a, p):
    """The stop test over the weighted sets from f recomputed in numpy FP64, the boxes, the equality."""
    box = p.box(y)
    f = K @ (a * y) - y
    hi = ((y == 1) & (a < box - p.eps)) | ((y == -1) & (a > p.eps))
    lo = ((y == 1) & (a > p.eps)) | ((y == -1) & (a < box - p.eps))
    gap = f[lo].max() - f[hi].min()
    print(f"weighted KKT gap {gap:.3e} (bound {2 * p.tau + 1e-9:.3e}), max alpha {a.max():.6g}")
    assert gap <= 2 * p.tau + 1e-9
    assert np.all(a >= -1e-9 * box) and np.all(a <= box * (1 + 1e-9))
    assert abs(np.dot(a, y)) <= 1e-9 * max(1.0, a.sum())
    assert np.any(a > p.C), "no alpha above C: the weights did not take effect"


# ---- 1. the weighted pairwise oracle against scikit-learn's solution -------------------------------------
@pytest.mark.parametrize("pair", ["A", "B"])
def test_pairwise_oracle_matches_the_sklearn_fixture(problems, pair):
    pr = problems[600]
    z = np.load(GOLDEN, allow_pickle=False)
    assert np.array_equal(z[f"weights_{pair}"], PAIRS[pair])
    a_ref, b_ref = z[f"alpha_{pair}"], -float(z[f"intercept_{pair}"])  # decision = sum alpha y K - b
    p = _params(PAIRS[pair])
    a, r, _ = C.smo_train(pr.X, pr.y, p)  # the svm_smo_train path (rows, not a kernel matrix)
    assert r.stop_reason == "converged"
    has_bounded_and_free_in_both_classes(pr.y, a, p)
    has_bounded_and_free_in_both_classes(pr.y, a_ref, p)
    o, o_ref = objective(pr.K, pr.y, a), objective(pr.K, pr.y, a_ref)
    print(f"pair {pair}: objective {o:.12f} fixture {o_ref:.12f} rel {abs(o - o_ref) / abs(o_ref):.3e}; "
          f"b {r.b:.9f} fixture {b_ref:.9f} diff {abs(r.b - b_ref):.3e}")
    assert abs(o - o_ref) <= 1e-8 * abs(o_ref)
    assert abs(r.b - b_ref) <= 4 * TAU


# ---- 2. an independent KKT check of both oracles ---------------------------------------------------------
@pytest.mark.parametrize("n", [600, 2000])
@pytest.mark.parametrize("pair", ["A", "B"])
@pytest.mark.parametrize("solver", ["pairwise", "decomp"])
def test_oracles_meet_the_weighted_kkt_conditions(problems, n, pair, solver):
    pr = problems[n]
    p = _params(PAIRS[pair])
    if solver == "pairwise":
        a, r, _ = C.smo_train_gram(pr.K, pr.y, p)
    else:
        a, r, _, _ = C.decomp_train_gram(pr.K, pr.y, p)
    assert r.stop_reason == "converged"
    has_bounded_and_free_in_both_classes(pr.y, a, p)
    kkt_checks(pr.K, pr.y, a, p)


@pytest.mark.parametrize("kw", [{"wss": 2}, {}], ids=["second-order", "warm"])
def test_pairwise_oracle_second_order_and_warm_start_under_weights(problems, kw):
    pr = problems[600]
    p = _params(PAIRS["A"], **kw)
    start = None
    if not kw:  # warm: the weighted solution of a looser problem is a feasible start
        start, _, _ = C.smo_train_gram(pr.K, pr.y, _params(PAIRS["A"], tau=1e-2))
        assert np.any(start > p.C)
    a, r, _ = C.smo_train_gram(pr.K, pr.y, p, alpha=start, warm=start is not None)
    assert r.stop_reason == "converged"
    kkt_checks(pr.K, pr.y, a, p)


@pytest.mark.parametrize("inner_wss", [1, 2])
def test_decomp_oracle_other_rules_and_warm_start_under_weights(problems, inner_wss):
    pr = problems[600]
    p = _params(PAIRS["B"])
    start, _, _, _ = C.decomp_train_gram(pr.K, pr.y, _params(PAIRS["B"], tau=1e-2), inner_wss=inner_wss)
    a, r, _, _ = C.decomp_train_gram(pr.K, pr.y, p, alpha=start, q=64, inner_wss=inner_wss)
    assert r.stop_reason == "converged"
    kkt_checks(pr.K, pr.y, a, p)


# ---- 3. equal weights are the unweighted bits ------------------------------------------------------------
def _raw_fit(fn_name, K, y, struct, decomp):
    a = np.zeros(len(y))
    r = N.SvmResult()
    if decomp:
        N.check(N.core().svm_decomp_train_gram(N.ptr(K), K.shape[1], N.ptr(y), len(y), N.ptr(a), 0, ctypes.byref(struct),
                                               1024, 0.1, 3, ctypes.byref(r), None, None), fn_name)
    else:
        N.check(N.core().svm_smo_train_gram(N.ptr(K), K.shape[1], N.ptr(y), len(y), N.ptr(a), 0, ctypes.byref(struct),
                                            ctypes.byref(r), None, 0), fn_name)
    return a, SMOResult.from_struct(r)


@pytest.mark.parametrize("decomp", [False, True], ids=["pairwise", "decomp"])
def test_equal_weights_are_the_unweighted_bits(problems, decomp):
    pr = problems[600]
    name = "svm_decomp_train_gram" if decomp else "svm_smo_train_gram"
    a0, r0 = _raw_fit(name, pr.K, pr.y, SVMParams(n_threads=4).to_struct(), decomp)
    a1, r1 = _raw_fit(name, pr.K, pr.y, SVMParams(n_threads=4, weight_pos=1, weight_neg=1).to_struct(), decomp)
    zeroed = N.params_struct(n_threads=4, weight_pos=0.0, weight_neg=0.0)  # an older caller's zero-filled tail
    assert zeroed.weight_pos == 0.0 and zeroed.weight_neg == 0.0
    a2, r2 = _raw_fit(name, pr.K, pr.y, zeroed, decomp)
    for a, r in ((a1, r1), (a2, r2)):
        assert np.array_equal(a, a0) and r.b == r0.b and r.iterations == r0.iterations
    assert r0.iterations > 100 and np.count_nonzero(a0) > 10


# ---- 4. the scaling identity -----------------------------------------------------------------------------
@pytest.mark.parametrize("decomp", [False, True], ids=["pairwise", "decomp"])
def test_weights_2_2_at_C5_are_C10_bit_for_bit(problems, decomp):
    pr = problems[600]
    name = "svm_decomp_train_gram" if decomp else "svm_smo_train_gram"
    a0, r0 = _raw_fit(name, pr.K, pr.y, SVMParams(n_threads=4, C=10.0).to_struct(), decomp)
    a1, r1 = _raw_fit(name, pr.K, pr.y, SVMParams(n_threads=4, C=5.0, weight_pos=2.0, weight_neg=2.0).to_struct(), decomp)
    assert np.array_equal(a1, a0) and r1.b == r0.b and r1.iterations == r0.iterations


# ---- 5. "balanced" ---------------------------------------------------------------------------------------
def test_balanced_resolves_to_n_over_2nc_and_equals_the_explicit_dict(problems):
    pr = problems[600]
    n, n_pos = len(pr.y), int((pr.y == 1).sum())
    wp, wn = resolve_class_weight("balanced", pr.y)
    assert wp == n / (2.0 * n_pos) and wn == n / (2.0 * (n - n_pos))
    g = SVC(class_weight="balanced", device="cpu").fit(pr.raw, pr.y)
    e = SVC(class_weight={1: wp, -1: wn}, device="cpu").fit(pr.raw, pr.y)
    assert g.class_weight_ == {1: wp, -1: wn} == e.class_weight_
    assert np.array_equal(g.alpha_, e.alpha_) and g.b_ == e.b_ and g.n_iter_ == e.n_iter_
    assert g.alpha_.max() > g.params.C  # the minority class's box is wider than C
    with pytest.raises(ValueError, match="class -1 is absent"):
        SVC(class_weight="balanced", device="cpu").fit(pr.raw[:5], np.ones(5, dtype=np.int32))
    with pytest.raises(ValueError, match=r"class \+1 is absent"):
        resolve_class_weight("balanced", -np.ones(5, dtype=np.int32))


def test_one_vs_rest_balanced_on_the_cpu_equals_per_class_solves():
    """Every class solve is the pairwise oracle on the shared kernel matrix with that class's balanced weights."""
    ds = synthetic_mnist(300, seed=77)
    m = OneVsRestSVC(class_weight="balanced", device="cpu").fit(ds.X, ds.labels, classes=[0, 1])
    Xs = MinMaxScaler().fit_transform(ds.X)
    K = C.rbf_matrix(Xs, Xs, m.params.gamma, m.params.n_threads)
    for k, c in enumerate(m.classes_):
        y = np.where(ds.labels == c, 1, -1).astype(np.int32)
        wp, wn = resolve_class_weight("balanced", y)
        assert m.class_weight_[k] == {1: wp, -1: wn} and wp > 1.0 > wn
        a, r, _ = C.smo_train_gram(K, y, m.params.replace(weight_pos=wp, weight_neg=wn))
        assert np.array_equal(m.dual_coef_[:, k], (a * y)[m.support_]) and m.intercepts_b_[k] == r.b
        assert set(np.flatnonzero(a > m.params.sv_tol)) <= set(m.support_)
        assert a.max() > m.params.C
        u, _, _ = C.smo_train_gram(K, y, m.params)
        assert not np.array_equal(u, a)  # and not the unweighted solve


# ---- 6. validation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_bad_weights_raise(problems, bad):
    with pytest.raises(ValueError, match="weight_pos"):
        SVMParams(weight_pos=bad)
    with pytest.raises(ValueError, match="weight_neg"):
        SVMParams(weight_neg=bad)
    with pytest.raises(ValueError, match="finite and > 0"):
        SVC(class_weight={1: bad, -1: 1.0}, device="cpu")
    if bad != 0.0:  # in the C struct 0 reads as 1; everything else out of range is SVM_ERR_ARG
        pr = problems[600]
        for decomp in (False, True):
            with pytest.raises(N.NativeError, match="class weights must be finite and > 0"):
                _raw_fit("fit", pr.K, pr.y, N.params_struct(weight_pos=bad), decomp)


@pytest.mark.parametrize("cw", [{1: 2.0}, {1: 2.0, 0: 1.0}, {1: 1.0, -1: 1.0, 2: 1.0}, "balance", 2.0, [2.0, 0.5]])
def test_bad_class_weight_forms_raise(cw):
    with pytest.raises(ValueError, match="class_weight"):
        SVC(class_weight=cw, device="cpu")


def test_warm_start_is_checked_against_the_class_boxes(problems):
    pr = problems[600]
    y = pr.y
    p = _params(PAIRS["A"])
    i, j = int(np.flatnonzero(y == 1)[0]), int(np.flatnonzero(y == -1)[0])
    a0 = np.zeros(len(y))
    a0[i] = a0[j] = 4.0  # feasible: both inside their boxes (20 and 5), sum(alpha y) = 0
    check_warm_start(a0, y, p.box(y))
    pos = np.flatnonzero(y == 1)[:5]
    neg = np.flatnonzero(y == -1)[:5]
    a1 = np.zeros(len(y))
    a1[pos[0]] = 15.0      # between C = 10 and C * weight_pos = 20 on a positive row
    a1[neg[:5]] = 3.0      # 5 negative rows at 3.0 <= C * weight_neg = 5 balance it
    SVC(class_weight={1: 2.0, -1: 0.5}, device="cpu").fit(pr.raw, y, alpha0=a1)
    with pytest.raises(ValueError, match="alpha0"):
        SVC(device="cpu").fit(pr.raw, y, alpha0=a1)  # unweighted: 15 > C
    a2 = np.zeros(len(y))
    a2[neg[0]] = a2[pos[0]] = 6.0  # 6 > C * weight_neg = 5 on a negative row
    with pytest.raises(ValueError, match="alpha0"):
        SVC(class_weight={1: 2.0, -1: 0.5}, device="cpu").fit(pr.raw, y, alpha0=a2)


# ---- 7. refusals, before any device is touched -----------------------------------------------------------
A = {1: 2.0, -1: 0.5}


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the device library or of torch.cuda fails the test: the refusals come first."""
    def boom(*a, **k):
        raise AssertionError("the device was touched before the refusal")

    monkeypatch.setattr(N, "hip", boom)
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "synchronize", boom)


@pytest.mark.parametrize("kw", [dict(solver="smo"), dict(shrinking=True), dict(wss="second"), dict(gram="fp64"),
                                dict(kcache="rows")], ids=lambda kw: next(iter(kw)))
def test_svc_refuses_weights_with_what_is_unweighted(problems, no_device, kw):
    pr = problems[600]
    with pytest.raises(ValueError, match="class weights"):
        SVC(device="cuda", class_weight=A, **kw).fit(pr.raw, pr.y)
    SVC(device="cuda", class_weight={1: 1.0, -1: 1.0}, **kw)  # weights of 1 are no weights


def test_shrinking_refuses_weights_on_the_cpu_oracle_too(problems):
    pr = problems[600]
    with pytest.raises(N.NativeError, match="class weights are not supported with shrinking"):
        C.decomp_train_gram(pr.K, pr.y, _params(PAIRS["A"], shrinking=True))
    with pytest.raises(ValueError, match="class weights"):
        SVC(device="cpu", class_weight=A, shrinking=True).fit(pr.raw, pr.y)


def test_newton_polish_refuses_weights_on_the_cpu_oracle(problems, monkeypatch):
    pr = problems[600]
    monkeypatch.setenv("SVM355_DECOMP_NEWTON", "1")
    with pytest.raises(N.NativeError, match="class weights are not supported with the Newton polish"):
        C.decomp_train_gram(pr.K, pr.y, _params(PAIRS["A"]))
    C.decomp_train_gram(pr.K, pr.y, _params())  # unweighted: still runs


@pytest.mark.parametrize("solver", ["batched", "streams"])
def test_one_vs_rest_pairwise_solvers_refuse_weights(no_device, solver):
    with pytest.raises(ValueError, match="class_weight"):
        OneVsRestSVC(solver=solver, class_weight="balanced", device="cuda")
    with pytest.raises(ValueError, match="class_weight"):
        OneVsRestSVC(class_weight={1: 2.0, -1: 0.5})


def test_distributed_trainers_refuse_weights(problems, no_device):
    from svm355.parallel.cascade import CascadeSVM
    from svm355.parallel.decomp import DistributedDecompSVC, group_fit
    from svm355.parallel.dsmo import DsmoGroup

    pr = problems[600]
    with pytest.raises(ValueError, match="class_weight"):
        DistributedDecompSVC(world=2, class_weight=A)
    with pytest.raises(ValueError, match="class weights"):
        group_fit(None, pr.raw, pr.y, _params(PAIRS["A"]))
    with pytest.raises(ValueError, match="class weights"):
        CascadeSVM(_params(PAIRS["A"])).fit(pr.raw, pr.y, world=2, device="cuda")
    with pytest.raises(ValueError, match="class weights"):
        DsmoGroup.fit(object.__new__(DsmoGroup), pr.raw.astype(np.uint8), pr.y, _params(PAIRS["A"]))


# ---- 8. persistence and the serial CLI -------------------------------------------------------------------
def test_save_load_keeps_the_weights_and_the_decisions(problems, tmp_path):
    pr = problems[600]
    g = SVC(class_weight=A, device="cpu").fit(pr.raw, pr.y)
    g.save(tmp_path / "m")
    info = json.loads((tmp_path / "m" / "model.json").read_text())
    assert info["params"]["weight_pos"] == 2.0 and info["params"]["weight_neg"] == 0.5
    h = SVC.load(tmp_path / "m")
    assert h.class_weight_ == g.class_weight_ == {1: 2.0, -1: 0.5}
    assert h.params.weight_pos == 2.0 and h.params.weight_neg == 0.5
    assert np.array_equal(h.decision_function(pr.raw[:50]), g.decision_function(pr.raw[:50]))
    # a model written before class weights existed: no such keys, weights of 1
    for k in ("weight_pos", "weight_neg"):
        del info["params"][k]
    (tmp_path / "m" / "model.json").write_text(json.dumps(info))
    old = SVC.load(tmp_path / "m")
    assert old.class_weight_ == {1: 1.0, -1: 1.0} and old.class_weight is None
    assert np.array_equal(old.decision_function(pr.raw[:50]), g.decision_function(pr.raw[:50]))


def _serial():
    exe = ROOT / "svm355" / "bin" / "svm_serial"
    if not exe.exists():
        from svm355 import build

        build.build_core()
        build.build_apps()
    return exe


def test_serial_cli_honours_the_weights(problems, tmp_path):
    pr = problems[600]
    out = tmp_path / "serial.json"
    r = subprocess.run([str(_serial()), "--synthetic", "600,100", "--seed", "77", "--weight-pos", "2", "--weight-neg",
                        "0.5", "--json", str(out), "--quiet"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    j = json.loads(out.read_text())
    g = SVC(class_weight=A, device="cpu").fit(pr.raw, pr.y)
    assert j["weight_pos"] == 2.0 and j["weight_neg"] == 0.5
    assert j["iterations"] == g.n_iter_ and j["n_sv"] == len(g.support_) and j["b"] == g.b_
    u = SVC(device="cpu").fit(pr.raw, pr.y)
    assert j["iterations"] != u.n_iter_  # and not the unweighted fit


@pytest.mark.parametrize("flag", ["--weight-pos", "--weight-neg"])
@pytest.mark.parametrize("value", ["0", "-1", "nan", "inf"])
def test_serial_cli_rejects_bad_weights(flag, value, tmp_path):
    r = subprocess.run([str(_serial()), "--synthetic", "50,10", flag, value], capture_output=True, text=True)
    assert r.returncode != 0
    assert f"{flag} must be finite and > 0" in r.stderr


def test_cli_help_lists_the_weights():
    r = subprocess.run([str(_serial()), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--weight-pos" in r.stderr and "--weight-neg" in r.stderr
