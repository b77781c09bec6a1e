"""The distance kernel block (decomp_dist.hip) against a longdouble reference at its tile edges (64 rows; 8 / 32 columns)."""
import numpy as np
import pytest
import torch

from svm355 import SVMParams
from svm355.ops import device as D

from dist_checks import U, kernel_ref, rows_with_zeros

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(1, 1), (63, 7), (64, 8), (65, 9), (63, 31), (64, 32), (65, 33), (130, 41), (41, 130)]


@pytest.mark.parametrize("d", [1, 15, 16, 17, 40])
@pytest.mark.parametrize("kernel", ["laplacian", "chi2"])
def test_store_against_longdouble_and_symmetry(kernel, d):
    kw = dict(kernel=kernel, gamma=2.0 / d)  # -gamma D in [-2, 0]: the range EXP_DEV was measured on
    p = SVMParams(**kw)
    X = rows_with_zeros(130, d, 100 * d + len(kernel))
    Xd = D.upload_rows(X, DEV)
    for m, n in SHAPES:
        out = torch.full((m + 1, n + 3), float("nan"), dtype=torch.float64, device=DEV)  # a spare row, spare columns
        K = D.dist_block(Xd[:m].contiguous(), Xd[:n].contiguous(), p, out=out).cpu().numpy()
        assert np.isnan(K[m]).all() and np.isnan(K[:, n:]).all(), (kernel, d, m, n)  # no tile overruns
        ref, bound = kernel_ref(X[:m], X[:n], **kw)
        assert np.all(np.abs(K[:m, :n] - ref) <= bound), (kernel, d, m, n)  # an unwritten element is NaN and fails
    K = D.dist_block(Xd, Xd, p)
    assert torch.equal(K, K.T.contiguous()) and bool((K.diagonal() == 1.0).all())


@pytest.mark.parametrize("n", [1, 129, 300])
@pytest.mark.parametrize("kernel", ["laplacian", "chi2"])
def test_sum_epilogues(kernel, n):
    kw = dict(kernel=kernel, gamma=2.0 / 17)
    p = SVMParams(**kw)
    rng = np.random.default_rng(n + len(kernel))
    X, B = rows_with_zeros(n, 17, n), rows_with_zeros(1024, 17, n + 1)
    coef, f0 = rng.uniform(-10.0, 10.0, 1024), rng.normal(size=2 * n)
    Xd, Bd, cd = D.upload_rows(X, DEV), D.upload_rows(B, DEV), torch.from_numpy(coef).to(DEV)
    ref, kb = kernel_ref(X, B, **kw)

    def run(epi, cnt, gate=0, start=None):
        f = torch.from_numpy((f0[: n * (2 if epi == "sum_twin" else 1)] if start is None else start).copy()).to(DEV)
        return D.dist_block(Xd, Bd, p, epi, coef=cd, f=f, count=cnt, gate=gate).cpu().numpy()

    np.testing.assert_array_equal(run("sum", 0), f0[:n])  # a count of 0 and a stopped solve's launch are no-ops
    np.testing.assert_array_equal(run("sum", 129, gate=1), f0[:n])
    for cnt in (1, 127, 128, 129, 1024):
        zero = run("sum", cnt, start=np.zeros(n))  # into f = 0 (the add into f is exact) against the longdouble sum
        want = ref[:, :cnt].astype(np.longdouble) @ coef[:cnt]
        bound = (cnt + 4) * U * np.abs(coef[:cnt] * ref[:, :cnt]).sum(1) + kb[:, :cnt] @ np.abs(coef[:cnt])
        assert np.all(np.abs(zero - want).astype(np.float64) <= bound), (kernel, n, cnt)
        out = run("sum", cnt)
        np.testing.assert_array_equal(out, f0[:n] + zero)  # into a non-zero f: the same sum, one add
        np.testing.assert_array_equal(run("sum", cnt), out)  # two runs, the same bits
        tw = run("sum_twin", cnt)  # the same sum into f[k] and f[k + n]: the plain form from each half's start
        np.testing.assert_array_equal(tw[:n], out)
        np.testing.assert_array_equal(tw[n:], run("sum", cnt, start=f0[n:]))
