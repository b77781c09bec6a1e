"""The pairwise-coupling kernel (csrc/hip/ovo_proba.hip, ``ops.device.ovo_couple``) against its host twin
``ops.cpu.ovo_couple`` -- bit for bit from given pair probabilities, within a measured bound with the sigmoid --
and the batched sigmoid fit (``ops.device.platt_fit_batch``) against ``ops.device.platt_fit`` segment by segment."""
import numpy as np
import pytest
import torch

from svm355 import _native as N
from svm355.ops import cpu as C
from svm355.ops import device as D

from ovo_proba_checks import (MIN_PROB, SIGMOID_TOL, check_invariants, extreme_case, mixed_sweeps_block,
                              pair_probabilities, sigmoid_cases, sigmoid_r)
from probability_checks import synthetic_pairs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _run_padded(r, A=None, B=None, pad=3):
    """The kernel on a row-strided view (ldd = P + pad) into NaN-filled outputs with ldp = k + pad and one spare
    row.  Returns (proba, label, iters) of the m rows as numpy after checking that nothing else was written."""
    m, P = r.shape
    k = int(round((1 + (1 + 8 * P) ** 0.5) / 2))
    wide = torch.full((m, P + pad), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :P] = torch.from_numpy(r).to(DEV)
    pw = torch.full((m + 1, k + pad), float("nan"), dtype=torch.float64, device=DEV)
    label = torch.full((m + 1,), -7, dtype=torch.int32, device=DEV)
    iters = torch.full((m + 1,), -7, dtype=torch.int32, device=DEV)
    Ad = None if A is None else torch.from_numpy(A).to(DEV)
    Bd = None if B is None else torch.from_numpy(B).to(DEV)
    D.ovo_couple(wide[:, :P], Ad, Bd, proba=pw[:, :k], label=label, iters=iters)
    pw, label, iters = pw.cpu().numpy(), label.cpu().numpy(), iters.cpu().numpy()
    assert np.all(np.isnan(pw[:m, k:])) and np.all(np.isnan(pw[m]))  # no stray store
    assert label[m] == -7 and iters[m] == -7
    return pw[:m, :k], label[:m], iters[:m]


@pytest.mark.parametrize("k", [2, 3, 5, 33, 63, 64])
@pytest.mark.parametrize("m", [1, 3, 4, 5, 257])
def test_coupling_from_given_r_is_the_twin_bit_for_bit(k, m):
    r = pair_probabilities(m, k, 1000 * k + m)
    want, wlabel, witers = C.ovo_couple(r)
    proba, label, iters = _run_padded(r)
    assert not np.any(np.isnan(proba))  # no missing store
    np.testing.assert_array_equal(proba, want)
    np.testing.assert_array_equal(iters, witers)
    np.testing.assert_array_equal(label, wlabel)
    np.testing.assert_array_equal(label, np.argmax(want, 1))  # the first maximum


@pytest.mark.parametrize("k", [3, 5, 33, 64])
def test_rows_of_one_workgroup_with_different_sweep_counts_end(k):
    """Consecutive rows -- waves of one workgroup up to 32 classes -- whose sweep counts differ: nothing in the
    per-row iteration waits for another row."""
    r = mixed_sweeps_block(k, 9, 7 + k)
    want, wlabel, witers = C.ovo_couple(r)
    for g in range(0, 8, 4):  # every aligned group of four rows holds different counts
        assert len(set(witers[g:g + 4].tolist())) > 1, witers
    proba, label, iters = _run_padded(r)
    np.testing.assert_array_equal(iters, witers)
    np.testing.assert_array_equal(proba, want)
    np.testing.assert_array_equal(label, wlabel)


@pytest.mark.parametrize("k", [2, 3, 33])
def test_nan_row_comes_out_nan_and_alone(k):
    r = pair_probabilities(6, k, 40 + k)
    r[2, 0] = np.nan
    want, _, witers = C.ovo_couple(r)
    proba, label, iters = _run_padded(r)
    assert np.all(np.isnan(proba[2])) and iters[2] == (0 if k == 2 else max(100, k))
    np.testing.assert_array_equal(iters, witers)
    keep = [0, 1, 3, 4, 5]
    np.testing.assert_array_equal(proba[keep], want[keep])


def test_contiguous_call_and_no_label():
    r = pair_probabilities(10, 4, 5)
    proba, label, iters = D.ovo_couple(torch.from_numpy(r).to(DEV), want_label=False)
    assert label is None
    np.testing.assert_array_equal(proba.cpu().numpy(), C.ovo_couple(r)[0])
    proba, label, iters = D.ovo_couple(torch.from_numpy(r[:0]).to(DEV))
    assert proba.shape == (0, 4)


@pytest.mark.parametrize("case", sigmoid_cases(), ids=lambda c: c[0])
def test_coupling_with_the_sigmoid_against_the_twin(case):
    """The device's exp is not the host's: within SIGMOID_TOL (10 x the measured difference) of the twin on the
    same (dec, A, B), and the derived invariants beside it."""
    name, dec, A, B = case
    k = int(round((1 + (1 + 8 * dec.shape[1]) ** 0.5) / 2))
    want, wlabel, witers = C.ovo_couple(dec, A, B)
    proba, label, iters = _run_padded(dec, A, B)
    diff = float(np.abs(proba - want).max())
    print(f"{name}: max |device - twin| = {diff:.3e} (bound {SIGMOID_TOL:.3e}); rows with another sweep count: "
          f"{int((iters != witers).sum())}")
    assert diff <= SIGMOID_TOL
    check_invariants(proba, sigmoid_r(dec, A, B), k, iters)


def test_extreme_decisions_stay_finite():
    dec, A, B = extreme_case(4)
    want = C.ovo_couple(dec, A, B)[0]
    proba, label, iters = _run_padded(dec, A, B)
    check_invariants(proba, sigmoid_r(dec, A, B), 4, iters)
    assert np.abs(proba - want).max() <= SIGMOID_TOL
    p2 = _run_padded(np.array([[800.0], [-800.0]]), np.array([-1.0]), np.array([0.0]))[0]
    np.testing.assert_array_equal(p2, [[1.0 - MIN_PROB, 1.0 - (1.0 - MIN_PROB)], [MIN_PROB, 1.0 - MIN_PROB]])


def test_coupling_refuses_bad_arguments():
    r = torch.from_numpy(pair_probabilities(4, 3, 1)).to(DEV)
    with pytest.raises(ValueError):
        D.ovo_couple(torch.ones((2, 4), dtype=torch.float64, device=DEV))  # no k (k - 1) / 2
    with pytest.raises(ValueError):
        D.ovo_couple(r, A=torch.ones(3, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        D.ovo_couple(r.float())
    ctx = D.DeviceContext.get(DEV)
    out = torch.empty((4, 3), dtype=torch.float64, device=DEV)
    for k, ldd, ldp in ((1, 3, 3), (65, 3000, 65), (3, 2, 3), (3, 3, 2)):
        rc = ctx.lib.svmd_ovo_couple(ctx.bind(), N.ptr(r), ldd, 4, k, None, None, N.ptr(out), ldp, None, None)
        assert rc != 0, (k, ldd, ldp)
    assert ctx.lib.svmd_ovo_couple(ctx.bind(), None, 3, 4, 3, None, None, N.ptr(out), 3, None, None) != 0


# ------------------------------------------------------------------ the batched sigmoid
SEGMENTS = (1, 2, 63, 64, 65, 1024, 1025, 8192, 8193)


def _segments(lengths, seed=0):
    decs, ys = zip(*(synthetic_pairs(n, seed + 10 * i) for i, n in enumerate(lengths)))
    off = np.concatenate([[0], np.cumsum(lengths)])
    return (torch.from_numpy(np.concatenate(decs)).to(DEV), torch.from_numpy(np.concatenate(ys)).to(DEV), off)


def _single(dec, y, off, use=None):
    return [D.platt_fit(dec[a:b].contiguous(), y[a:b].contiguous(), None if use is None else use[a:b].contiguous())
            for a, b in zip(off[:-1], off[1:])]


def test_batch_is_the_single_fit_segment_by_segment():
    dec, y, off = _segments(SEGMENTS)
    got = D.platt_fit_batch(dec, y, off)
    want = _single(dec, y, off)
    assert got == want  # A, B, iterations and status, bit for bit
    assert got[0].status == "degenerate" and all(g.status == "converged" for g in got[2:])  # n = 1: one class


def test_batch_with_a_use_mask():
    dec, y, off = _segments(SEGMENTS, seed=3)
    use = torch.from_numpy((np.random.default_rng(1).random(dec.shape[0]) < 0.7).astype(np.uint8)).to(DEV)
    use[off[:-1].tolist()] = 1
    assert D.platt_fit_batch(dec, y, off, use=use) == _single(dec, y, off, use)


def test_batch_degenerate_segment_in_the_middle():
    dec, y, off = _segments((300, 200, 301), seed=5)
    clean = D.platt_fit_batch(dec, y, off)
    y2 = y.clone()
    y2[300:500] = 1  # one class only
    got = D.platt_fit_batch(dec, y2, off)
    assert got[1].status == "degenerate" and got[1].iterations == 0 and got[1].A == 0.0
    assert got[0] == clean[0] and got[2] == clean[2]
    assert got == _single(dec, y2, off)


def test_batch_of_one():
    dec, y, off = _segments((500,), seed=8)
    assert D.platt_fit_batch(dec, y, off) == [D.platt_fit(dec, y)]
    # a segment inside a longer buffer
    assert D.platt_fit_batch(dec, y, [100, 400]) == _single(dec, y, np.array([100, 400]))


def test_batch_refuses_bad_offsets():
    dec, y, off = _segments((50, 60), seed=9)
    for bad in ([0, 50, 50, 110], [0, 60, 50], [-1, 50, 110], [0, 50, 111], [0], [[0, 50]]):
        with pytest.raises(ValueError):
            D.platt_fit_batch(dec, y, bad)
    ctx = D.DeviceContext.get(DEV)
    out = (N.SvmPlatt * 2)()
    for bad in ([0, 50, 50], [5, 3, 60], [-2, 50, 110]):
        o = np.array(bad, dtype=np.int64)
        assert ctx.lib.svmd_platt_fit_batch(ctx.bind(), N.ptr(dec), N.ptr(y), None, N.ptr(o), 2, out) != 0
    assert ctx.lib.svmd_platt_fit_batch(ctx.bind(), N.ptr(dec), N.ptr(y), None, None, 2, out) != 0
