"""The estimators' shared plumbing (svm355/models/_device.py) and the pool's shape rule, at n = 33, d = 17: a row
stride padded to 32 with one ragged 16-wide tail, the smallest shape at which the padding, the widening of byte
rows and the support-vector gather can each go wrong.  The rows are integers in 0..255, so their byte and FP64
forms hold the same values exactly."""
import numpy as np
import pytest

N, D = 33, 17


@pytest.fixture(scope="module")
def X8():
    X = np.random.default_rng(5).integers(0, 256, size=(N, D), dtype=np.uint8)
    assert np.all(X.min(0) < X.max(0))  # no constant column here (test_constant_column_and_nan has one)
    return X


def _raises(fn):
    with pytest.raises(ValueError) as e:
        fn()
    return str(e.value)


@pytest.mark.gpu
def test_train_rows_bytes_and_fp64(X8):
    import torch

    from svm355.models._device import TrainRows

    forms = [TrainRows.upload(X8, "cuda"), TrainRows.upload(X8.astype(np.float64), "cuda")]
    assert forms[0].rows.dtype == torch.uint8 and tuple(forms[0].rows.shape) == (N, D) and forms[0].sqn is None
    assert forms[1].rows.dtype == torch.float64 and tuple(forms[1].rows.shape) == (N, 32) and forms[1].sqn is not None
    for r in forms:
        assert np.array_equal(r.mn_h, X8.min(0).astype(np.float64))
        assert np.array_equal(r.mx_h, X8.max(0).astype(np.float64))
        assert np.array_equal(r.mn.cpu().numpy(), r.mn_h) and np.array_equal(r.mx.cpu().numpy(), r.mx_h)
        # the two halves of one 2 d buffer: one copy reads both back
        assert r.mn.untyped_storage().data_ptr() == r.mx.untyped_storage().data_ptr()
        assert r.mn.is_contiguous() and r.mx.is_contiguous() and r.mn.numel() == r.mx.numel() == D
        assert r.mx.storage_offset() == r.mn.storage_offset() + D
        assert r.d == D and r.upload_ms > 0
    for idx in ([0, 5, 32], list(range(N)), []):
        (Xa, na), (Xb, nb) = (r.sv(np.array(idx, dtype=np.int64)) for r in forms)
        assert tuple(Xa.shape) == (len(idx), 32) and tuple(na.shape) == (len(idx),)
        assert torch.equal(Xa, Xb) and torch.equal(na, nb)
        if idx:
            assert float(Xa.min()) >= 0.0 and float(Xa.max()) <= 1.0
            assert not Xa[:, D:].any()  # the padding is zero
            # D squares summed in FP64, in the kernel's order and in torch's: each within D ulp of the exact sum
            assert torch.allclose(na, (Xa * Xa).sum(1), rtol=4 * D * 2.0**-53, atol=0)
        if len(idx) == N:  # every column's minimum scales to 0 and its maximum to 1
            assert not Xa[:, :D].min(0).values.any() and bool((Xa[:, :D].max(0).values == 1.0).all())
            assert np.array_equal(Xa[:, :D].cpu().numpy() == 0.0, X8 == X8.min(0))


@pytest.mark.gpu
def test_constant_column_and_nan(X8):
    """What SVC(device="cuda").fit shows for a constant column (it scales to 0, no error) and for a NaN (a
    ValueError naming the column; without scaling, the plain one), TrainRows shows too."""
    from svm355 import SVC
    from svm355.models._device import TrainRows

    y = np.where(np.arange(N) % 2 == 0, 1, -1).astype(np.int32)
    Xc = X8.copy()
    Xc[:, 3] = 77
    for X in (Xc, Xc.astype(np.float64)):
        r = TrainRows.upload(X, "cuda")
        assert r.mn_h[3] == r.mx_h[3] == 77.0
        Xs, ns = r.sv(np.arange(N))
        assert not Xs[:, 3].any() and bool(np.isfinite(ns.cpu().numpy()).all())
        m = SVC(device="cuda").fit(X, y)
        assert m.scaler_.min_[3] == m.scaler_.max_[3] == 77.0 and not m.support_vectors_[:, 3].any()
    Xn = X8.astype(np.float64)
    Xn[4, 9] = np.nan
    want = "X holds NaN or infinite values (columns [9])"
    assert _raises(lambda: TrainRows.upload(Xn, "cuda")) == want
    assert _raises(lambda: SVC(device="cuda").fit(Xn, y)) == want
    want = "X holds NaN or infinite values"
    assert _raises(lambda: TrainRows.upload(Xn, "cuda", scale=False)) == want
    assert _raises(lambda: SVC(device="cuda", scale=False).fit(Xn, y)) == want
    r = TrainRows.upload(X8.astype(np.float64), "cuda", scale=False)
    assert r.mn is None and r.mx is None and r.mn_h is None and r.mx_h is None
    assert np.array_equal(r.sqn.cpu().numpy(), (X8.astype(np.float64) ** 2).sum(1))  # integers: exact


@pytest.mark.gpu
def test_loaded_model_without_support_vectors(X8, tmp_path):
    from svm355 import SVR

    z = np.linspace(0.0, 1.0, N)
    m = SVR(epsilon=10.0, device="cuda").fit(X8, z)  # the tube swallows every target
    assert len(m.support_) == 0
    m.save(tmp_path)
    g = SVR.load(tmp_path, device="cuda")
    assert tuple(g._dev["Xs"].shape) == (0, 32) and tuple(g._dev["ns"].shape) == (0,)
    for Xq in (X8[:7], X8[:7].astype(np.float64)):
        assert np.array_equal(g.predict(Xq), np.full(7, -g.b_))
    assert g.b_ == m.b_


@pytest.mark.gpu
def test_solve_on_rows_widens_declined_bytes(X8):
    import torch

    from svm355.models._device import solve_on_rows

    seen = []

    def decline_bytes(rows):
        seen.append(rows)
        return None if rows.sqn is None else "solved"

    rows, out = solve_on_rows(X8, "cuda", decline_bytes)
    assert out == "solved" and rows is seen[1] and len(seen) == 2
    assert seen[0].rows.dtype == torch.uint8 and rows.rows.dtype == torch.float64 and rows.sqn is not None
    assert np.array_equal(rows.mn_h, seen[0].mn_h) and np.array_equal(rows.mx_h, seen[0].mx_h)
    # the FP64 rows of the same values: scaled as the bytes' support-vector rows are
    assert torch.equal(rows.rows, seen[0].sv(np.arange(N))[0])
    seen.clear()
    assert solve_on_rows(X8, "cuda", lambda r: seen.append(r)) == (None, None)
    assert [r.sqn is None for r in seen] == [True, False]
    seen.clear()
    rows, out = solve_on_rows(X8, "cuda", lambda r: seen.append(r) or 1, bytes_ok=False)  # straight to FP64 rows
    assert out == 1 and len(seen) == 1 and rows.sqn is not None


def test_pool_shape():
    from svm355.models.multiclass import pool_shape

    small, big = (60000, 784), (1000000, 784)  # 45 MiB and 748 MiB of pixel rows: either side of 192 MiB
    assert small[0] * small[1] <= 192 << 20 < big[0] * big[1]
    assert pool_shape(10, None, *small) == (10, 0.05)  # all tasks side by side
    assert pool_shape(10, None, *big) == (2, 0.25)  # two at a time
    assert pool_shape(10, None, 256 << 10, 768) == (10, 0.05)  # exactly 192 MiB: not past it
    assert pool_shape(10, None, (256 << 10) + 1, 768) == (2, 0.25)
    for shape in (small, big):  # an explicit width wins on both sides, capped at the number of tasks
        assert pool_shape(10, 3, *shape) == (3, min(0.25, 0.5 / 3))
        assert pool_shape(10, 50, *shape) == (10, 0.05)
        assert pool_shape(1, None, *shape) == (1, 0.25)
    for n_tasks in range(1, 12):
        for cs in (None, 1, 2, 4, 16):
            for shape in (small, big):
                width, frac = pool_shape(n_tasks, cs, *shape)
                assert 1 <= width <= n_tasks and frac == min(0.25, 0.5 / width)
