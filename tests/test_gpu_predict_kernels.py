"""The prediction-path kernels at the shapes the rest of the suite never reaches.

Every estimator predicts through svmd_decision (the FP64 MFMA cross-kernel + the row GEMV), and every byte-path
model gets its support-vector rows from svmd_sv_rows_u8 and its statistics from svmd_minmax_u8.  These tests run
the arms that a comfortable shape never takes: a partial last band of the rectangular tile map, the full-grid
symmetric launch (SVM355_GRAM_TRI=0), a second chunk of svmd_decision, support-vector counts around a wave, row
counts below a block, widths that straddle a wave.

Unless a test says otherwise rows are uniform(0, 1), gamma = 0.5 / d, the reference is the direct-difference FP64
RBF of svm355.ops.cpu.rbf_matrix and the bound per kernel value is 2e-14 (test_rbf_gram_vs_fp64_reference's).
Outputs are pre-filled with NaN wherever the wrapper takes one, so an element nobody wrote cannot pass.
"""

import math

import numpy as np
import pytest
import torch

from svm355.ops import cpu as C
from svm355.utils.data import MinMaxScaler

pytestmark = pytest.mark.gpu

KTOL = 2e-14  # per kernel value


@pytest.fixture(scope="module")
def dev():
    from svm355.ops import device as D

    assert D.available(), "GPU visible but the HIP device library did not load"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def D():
    from svm355.ops import device as D

    return D


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=dev)


def _rows(D, dev, X, d):
    Xd = D.upload_rows(X, dev)
    return Xd, D.row_norms(Xd, d)


# ---------------------------------------------------------------- (a) the rectangular tile map
@pytest.mark.parametrize("m,n,d", [
    (1153, 257, 16),  # 10 x 3 tiles: last band of 2 row tiles, last row tile 1 row, last column tile 1 column; 30 workgroups
    (2049, 129, 33),  # 17 x 2 tiles: last band is a single row tile
    (1025, 1, 16),    # 9 x 1 tiles
])
def test_cross_kernel_writes_every_tile_and_nothing_else(dev, D, m, n, d):
    rng = np.random.default_rng(m + n + d)
    A = rng.uniform(0, 1, size=(m, d))
    B = rng.uniform(0, 1, size=(n, d))
    gamma = 0.5 / d
    (Ad, nA), (Bd, nB) = _rows(D, dev, A, d), _rows(D, dev, B, d)
    K = _nan((m + 1, n + 3), dev)  # three spare columns (row stride > n) and a spare row
    assert D.rbf_gram(Ad, nA, Bd, nB, gamma, out=K) is K
    Kh = K.cpu().numpy()
    unwritten = np.argwhere(np.isnan(Kh[:m, :n]))
    assert unwritten.size == 0, f"{len(unwritten)} elements never written, first at {unwritten[0]} (tile {unwritten[0] // 128})"
    np.testing.assert_allclose(Kh[:m, :n], C.rbf_matrix(A, B, gamma), rtol=0, atol=KTOL)
    assert np.isnan(Kh[:, n:]).all(), "written past column n"
    assert np.isnan(Kh[m]).all(), "written past row m"


# ---------------------------------------------------------------- (b) the symmetric launch, both arms
SYM_N, SYM_D = 1153, 16  # 10 row tiles: 55 workgroups in the triangular arm, 100 in the full one


@pytest.fixture(scope="module")
def sym_data(dev, D):
    X = np.random.default_rng(SYM_N + SYM_D).uniform(0, 1, size=(SYM_N, SYM_D))
    gamma = 0.5 / SYM_D
    return X, gamma, C.rbf_matrix(X, X, gamma), _rows(D, dev, X, SYM_D)


def _sym_gram(D, dev, sym_data, monkeypatch, arm):
    if arm == "tri":
        monkeypatch.delenv("SVM355_GRAM_TRI", raising=False)
    else:
        monkeypatch.setenv("SVM355_GRAM_TRI", "0")
    _, gamma, _, (Xd, nrm) = sym_data
    K = _nan((SYM_N, SYM_N + 3), dev)  # even row stride (the mirror stores are 16-byte pairs), three spare columns
    D.rbf_gram(Xd, nrm, Xd, nrm, gamma, symmetric=True, out=K)
    return K.cpu().numpy()


@pytest.mark.parametrize("arm", ["tri", "full"])
def test_symmetric_gram_arm_vs_fp64_reference(dev, D, sym_data, monkeypatch, arm):
    Kh = _sym_gram(D, dev, sym_data, monkeypatch, arm)
    K = Kh[:, :SYM_N]
    assert not np.isnan(K).any(), f"{np.isnan(K).sum()} elements never written"
    assert np.isnan(Kh[:, SYM_N:]).all(), "written past column n"
    assert np.all(np.diag(K) == 1.0)
    np.testing.assert_array_equal(K, K.T)  # exactly symmetric
    np.testing.assert_allclose(K, sym_data[2], rtol=0, atol=1e-13)  # test_rbf_gram_symmetric_diag_exact's bound


def test_symmetric_gram_arms_equal_bit_for_bit(dev, D, sym_data, monkeypatch):
    """An entry's arithmetic (its k order in the MFMA loop, the epilogue) does not depend on which workgroup owns
    its tile, and the triangular arm's mirrored half is a copy."""
    tri = _sym_gram(D, dev, sym_data, monkeypatch, "tri")
    full = _sym_gram(D, dev, sym_data, monkeypatch, "full")
    np.testing.assert_array_equal(tri[:, :SYM_N], full[:, :SYM_N])


# ---------------------------------------------------------------- (c) decision at the edges of the GEMV
DEC_D, DEC_B = 33, 0.75


def _decision_case(D, dev, nsv, m):
    rng = np.random.default_rng(1000 * nsv + m)
    Xs = rng.uniform(0, 1, size=(nsv, DEC_D))
    Xq = rng.uniform(0, 1, size=(m, DEC_D))
    coef = rng.uniform(-10, 10, nsv)
    return Xs, Xq, coef, _rows(D, dev, Xs, DEC_D), _rows(D, dev, Xq, DEC_D)


@pytest.mark.parametrize("m", [1, 127, 129])
@pytest.mark.parametrize("nsv", [1, 2, 63, 64, 65, 129])
def test_decision_small_sv_counts_vs_fp64_reference(dev, D, nsv, m):
    """nsv around one wave of the GEMV (a lane's stride is 64) and odd nsv (the scratch block's row stride is
    nsv rounded up to even: the pad column must not be summed); m around one 128-row tile and below one block of
    the GEMV.  Each kernel value may be 2e-14 off, so the sum may be 2e-14 * sum |coef| off; the reference sums in
    extended precision, and the device sum's own rounding is orders of magnitude below the bound."""
    Xs, Xq, coef, (Xsd, ns), (Xqd, nq) = _decision_case(D, dev, nsv, m)
    gamma = 0.5 / DEC_D
    out = D.decision(Xsd, ns, torch.from_numpy(coef).to(dev), Xqd, nq, gamma, DEC_B).cpu().numpy()
    ref = (C.rbf_matrix(Xq, Xs, gamma).astype(np.longdouble) @ coef.astype(np.longdouble) - DEC_B).astype(np.float64)
    assert out.shape == (m,)
    np.testing.assert_allclose(out, ref, rtol=0, atol=KTOL * np.abs(coef).sum())


@pytest.mark.parametrize("j", [0, 70, 128])
def test_decision_with_a_unit_coefficient_is_the_cross_kernels_column(dev, D, j):
    """coef = e_j, b = 0: the GEMV adds exact zeros to K[:, j], so the result is that column bit for bit."""
    nsv = m = 129
    _, _, _, (Xsd, ns), (Xqd, nq) = _decision_case(D, dev, nsv, m)
    gamma = 0.5 / DEC_D
    e = torch.zeros(nsv, dtype=torch.float64, device=dev)
    e[j] = 1.0
    out = D.decision(Xsd, ns, e, Xqd, nq, gamma, 0.0).cpu().numpy()
    K = D.rbf_gram(Xqd, nq, Xsd, ns, gamma).cpu().numpy()
    np.testing.assert_array_equal(out, K[:, j])


# ---------------------------------------------------------------- (d) more than one chunk of svmd_decision
CH_NSV, CH_D, CH_M = 4097, 16, 16385


def _decision_chunk_rows(nsv):
    """svmd_decision's rows per chunk (csrc/hip/capi.hip): what fits 512 MB of scratch, in whole 128-row tiles."""
    ldk = (nsv + 1) // 2 * 2
    return max(128, (512 << 20) // (ldk * 8) // 128 * 128)


@pytest.fixture(scope="module")
def chunked(dev, D):
    rng = np.random.default_rng(CH_NSV + CH_M)
    Xs = rng.uniform(0, 1, size=(CH_NSV, CH_D))
    Xq = rng.uniform(0, 1, size=(CH_M, CH_D))
    coef = rng.uniform(-10, 10, CH_NSV)
    gamma = 0.5 / CH_D
    (Xsd, ns), (Xqd, nq) = _rows(D, dev, Xs, CH_D), _rows(D, dev, Xq, CH_D)
    coefd = torch.from_numpy(coef).to(dev)
    out = D.decision(Xsd, ns, coefd, Xqd, nq, gamma, DEC_B)
    return dict(Xs=Xs, Xq=Xq, coef=coef, gamma=gamma, Xsd=Xsd, ns=ns, Xqd=Xqd, nq=nq, coefd=coefd, out=out)


def test_decision_chunk_size_still_makes_this_two_chunks():
    """Not a skip: a change of the chunk size must fail here, not quietly make the tests below single-chunk."""
    rows = _decision_chunk_rows(CH_NSV)
    assert rows == 16256
    assert CH_M > rows and CH_M - rows == 129  # a second chunk of two row tiles, the last with one row


def test_decision_second_chunk_vs_fp64_reference(dev, D, chunked):
    """All 16385 rows against the reference, in row blocks (the 16385 x 4097 reference never exists at once)."""
    assert CH_M > _decision_chunk_rows(CH_NSV)
    c = chunked
    out = c["out"].cpu().numpy()
    assert out.shape == (CH_M,)
    tol = KTOL * np.abs(c["coef"]).sum()
    coef_l = c["coef"].astype(np.longdouble)
    worst = 0.0
    for r0 in range(0, CH_M, 1024):
        Kb = C.rbf_matrix(c["Xq"][r0:r0 + 1024], c["Xs"], c["gamma"])
        ref = (Kb.astype(np.longdouble) @ coef_l - DEC_B).astype(np.float64)
        err = np.abs(out[r0:r0 + len(ref)] - ref)
        worst = max(worst, float(err.max()))
        assert err.max() <= tol, f"rows {r0}..{r0 + len(ref) - 1}: |error| {err.max():.3e} > {tol:.3e} at row {r0 + err.argmax()}"
    print(f"decision, two chunks: worst |error| {worst:.3e}, bound {tol:.3e}")


def test_decision_chunks_equal_their_rows_alone_bit_for_bit(dev, D, chunked):
    """A row's value depends on its own k order in the MFMA loop and on the GEMV's fixed butterfly, not on the
    rows computed with it: each chunk's rows equal a call on those query rows alone."""
    r0 = _decision_chunk_rows(CH_NSV)
    assert CH_M > r0
    c = chunked
    out = c["out"].cpu().numpy()
    tail = D.decision(c["Xsd"], c["ns"], c["coefd"], c["Xqd"][r0:], c["nq"][r0:], c["gamma"], DEC_B).cpu().numpy()
    np.testing.assert_array_equal(out[r0:], tail)
    head = D.decision(c["Xsd"], c["ns"], c["coefd"], c["Xqd"][:r0], c["nq"][:r0], c["gamma"], DEC_B).cpu().numpy()
    np.testing.assert_array_equal(out[:r0], head)


# ---------------------------------------------------------------- (e) sv_rows_u8 against the FP64 path
U8_N = 300


def _u8_rows(d, seed):
    """uint8 rows with a constant first column and a last column spanning 0..255 (d = 1: the spanning one)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, size=(U8_N, d), dtype=np.uint8)
    if d > 1:
        X[:, 0] = 7
    X[:, d - 1] = rng.permutation(np.arange(U8_N) % 256).astype(np.uint8)
    return X


def _index_lists(rng):
    """Lengths 0, 1, 3, 5, 130 (more than one block of 4 rows, a partial last block): unsorted, with repeats, rows 0
    and n - 1 included."""
    lists = [np.zeros(0, dtype=np.int64), np.array([0]), np.array([U8_N - 1])]
    for k in (3, 5, 130):
        idx = rng.integers(0, U8_N, k)
        idx[:3] = [U8_N - 1, 0, U8_N - 1]
        lists.append(idx.astype(np.int64))
    return lists


@pytest.mark.parametrize("extra", [0, 16, 80], ids=["ld=padded", "ld=padded+16", "ld=padded+80"])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 784])
def test_sv_rows_u8_equal_the_scaled_fp64_rows(dev, D, d, extra):
    """The rows and norms a byte-path model keeps are those of the widened, scaled FP64 matrix bit for bit, and the
    padding is zero: up to ld (a wider ld than the default gives the padding loop 16 + 80 columns, more than one
    pass of a wave, at d = 784 the only padding there is)."""
    X = _u8_rows(d, seed=d)
    ld = D.padded_dim(d) + extra
    Xu = D.upload_u8(X, dev)
    mm = _nan((2 * d,), dev)
    mn, mx = D.minmax_u8(Xu, out=mm)
    Xd = D.upload_rows(X, dev, ld=ld)  # widened on the device, zero padded
    mn64, mx64, sqn = D.minmax_scale_(Xd, d)
    np.testing.assert_array_equal(mn.cpu().numpy(), mn64.cpu().numpy())
    np.testing.assert_array_equal(mx.cpu().numpy(), mx64.cpu().numpy())
    Xd, sqn = Xd.cpu().numpy(), sqn.cpu().numpy()
    Xs = MinMaxScaler().fit(X).transform(X)
    assert Xs[:, 0].max() == 0.0 or d == 1  # the constant column scales to 0 (range falls back to 1)
    for idx in _index_lists(np.random.default_rng(d + extra)):
        k = len(idx)
        out = _nan((k, ld), dev)
        rows, nrm = D.sv_rows_u8(Xu, torch.from_numpy(idx).to(dev), mn, mx, ld=ld, out=out)
        assert rows is out and nrm.shape == (k,)
        rows, nrm = rows.cpu().numpy(), nrm.cpu().numpy()
        np.testing.assert_array_equal(rows, Xd[idx], err_msg=f"k = {k}")   # the whole padded width
        np.testing.assert_array_equal(nrm, sqn[idx], err_msg=f"k = {k}")
        np.testing.assert_array_equal(rows[:, :d], Xs[idx], err_msg=f"k = {k}")
        assert np.all(rows[:, d:] == 0.0), f"k = {k}: padding columns not zero"


def test_sv_rows_u8_constant_single_column(dev, D):
    """d = 1 and the one column constant: the range falls back to 1, every row and norm is exactly 0."""
    X = np.full((U8_N, 1), 9, dtype=np.uint8)
    Xu = D.upload_u8(X, dev)
    mn, mx = D.minmax_u8(Xu)
    idx = torch.tensor([U8_N - 1, 0, 5, 0], device=dev)
    out = _nan((4, 16), dev)
    rows, nrm = D.sv_rows_u8(Xu, idx, mn, mx, out=out)
    assert torch.all(rows == 0.0) and torch.all(nrm == 0.0)


# ---------------------------------------------------------------- (f) minmax_u8 against numpy
@pytest.mark.parametrize("d", [1, 63, 65, 784])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 4097])
def test_minmax_u8_vs_numpy(dev, D, n, d):
    """n < 4 leaves waves of the block without a row, n = 5 is two row partitions, the second with one wave of
    rows; d straddles a wave.  A wave that owns no row holds min 255 / max 0 and its any flag decides whether a
    partition's result counts at all (else +-inf): the column of 255s and the column of 0s are the data on which
    those defaults and the real values coincide, every other column the data on which they do not."""
    rng = np.random.default_rng(10 * n + d)
    base = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    variants = []
    if d > 1:
        base[:, 0] = 255
        base[:, d - 1] = 0
        variants.append(base)
    else:
        variants += [base, np.full((n, 1), 255, dtype=np.uint8), np.zeros((n, 1), dtype=np.uint8)]
    for X in variants:
        mm = _nan((2 * d,), dev)
        mn, mx = D.minmax_u8(D.upload_u8(X, dev), out=mm)
        np.testing.assert_array_equal(mn.cpu().numpy(), X.min(0).astype(np.float64))
        np.testing.assert_array_equal(mx.cpu().numpy(), X.max(0).astype(np.float64))


# ---------------------------------------------------------------- (g) minmax_scale_ / row_norms, small and straddling
@pytest.mark.parametrize("n,d", [(1, 1), (3, 63), (5, 64), (6, 65), (130, 129)])
def test_minmax_scale_and_row_norms_small_shapes(dev, D, n, d):
    """n below one block of 4 rows (waves that return early), a partial last block, d on both sides of a wave's 64
    lanes and past two passes.  Min, max and the scaled rows are exact (true division, as test_minmax_scale_norms);
    the norms are compared with the exactly rounded sum of the squares."""
    rng = np.random.default_rng(100 * n + d)
    X = rng.uniform(-3, 5, size=(n, d))
    Xd = D.upload_rows(X, dev)
    ld = Xd.shape[1]
    raw = D.row_norms(Xd, d).cpu().numpy()
    np.testing.assert_allclose(raw, [math.fsum(v * v for v in row) for row in X], rtol=1e-13, atol=0)
    mn, mx, sqn = D.minmax_scale_(Xd, d)
    sc = MinMaxScaler().fit(X)
    np.testing.assert_array_equal(mn.cpu().numpy(), sc.min_)
    np.testing.assert_array_equal(mx.cpu().numpy(), sc.max_)
    np.testing.assert_array_equal(mn.cpu().numpy(), X.min(0))
    np.testing.assert_array_equal(mx.cpu().numpy(), X.max(0))
    Xs = sc.transform(X)
    Xh = Xd.cpu().numpy()
    np.testing.assert_array_equal(Xh[:, :d], Xs)
    assert np.all(Xh[:, d:] == 0.0) and Xh.shape == (n, ld)
    want = np.array([math.fsum(v * v for v in row) for row in Xs])
    np.testing.assert_allclose(sqn.cpu().numpy(), want, rtol=1e-13, atol=0)
    np.testing.assert_allclose(D.row_norms(Xd, d).cpu().numpy(), want, rtol=1e-13, atol=0)
    if n == 1:  # every column constant: the range falls back to 1
        assert np.all(Xh == 0.0) and np.all(sqn.cpu().numpy() == 0.0)
