"""The precomputed-kernel device kernels (decomp_gram.hip) step by step: the streamed row sum against a numpy replay of
its order (bit for bit) and against math.fsum, the K(W, W) gather, the symmetry check, and the prediction gather."""
import math

import numpy as np
import pytest
import torch

from svm355.ops import device as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -53


def _device(K, extra=8):
    """K on the device as a view with a row stride strictly above its width (the padded upload's, plus 8)."""
    m, n = K.shape
    buf = torch.zeros((m, D.padded_gram_dim(n) + extra), dtype=torch.float64, device=DEV)
    buf[:, :n] = torch.from_numpy(K).to(DEV)
    return buf[:, :n]


def _replay(K, cols, coef, cnt):
    """rowsum_update_kfun's order: sixteen strided chains from 0.0, product rounded then added, the 8 4 2 1 tree."""
    v = np.zeros((16, K.shape[1]))
    for k in range(cnt):
        v[k % 16] = v[k % 16] + coef[k] * K[cols[k]]
    for off in (8, 4, 2, 1):
        v[:off] = v[:off] + v[off:2 * off]
    return v[0]


@pytest.mark.parametrize("twin", [False, True])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 511, 513])
def test_rowsum_replays_the_oracles_order_bit_for_bit(n, twin):
    rng = np.random.default_rng(n)
    K = rng.normal(size=(n, n))
    Kd = _device(K)
    assert Kd.stride(0) > n
    ncols = min(1024, n)
    cols = rng.permutation(n)[:ncols].astype(np.int32)
    coef = rng.normal(size=ncols)
    cd, fd = torch.from_numpy(cols).to(DEV), torch.from_numpy(coef).to(DEV)
    f0 = rng.normal(size=2 * n if twin else n)
    for cnt in sorted({min(c, n) for c in (0, 1, 15, 16, 17, 1024)}):
        got = D.gram_rowsum(Kd, cd, fd, torch.from_numpy(f0).to(DEV), cnt, twin=twin).cpu().numpy()
        s = _replay(K, cols, coef, cnt)
        want = f0 + np.tile(s, 2 if twin else 1) if cnt else f0  # a count of 0 writes nothing
        np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64), err_msg=f"cnt={cnt}")
    gated = D.gram_rowsum(Kd, cd, fd, torch.from_numpy(f0).to(DEV), ncols, gate=1, twin=twin).cpu().numpy()
    np.testing.assert_array_equal(gated.view(np.int64), f0.view(np.int64))
    # from f = 0 at the full count: the sum itself against math.fsum of the rounded products
    got = D.gram_rowsum(Kd, cd, fd, torch.zeros(len(f0), dtype=torch.float64, device=DEV), ncols, twin=twin).cpu().numpy()
    P = coef[:, None] * K[cols]
    ref = np.array([math.fsum(P[:, i]) for i in range(n)])
    bound = (ncols / 16 + 5) * U * np.abs(P).sum(0)
    err = np.abs(got - np.tile(ref, 2 if twin else 1))
    print(f"n={n} twin={twin}: max err / bound {np.max(err / np.tile(bound, 2 if twin else 1)):.3f}")
    assert np.all(err <= np.tile(bound, 2 if twin else 1))


@pytest.mark.parametrize("m,twin", [(1, False), (2, False), (64, False), (65, False), (1024, False), (65, True)])
def test_kww_is_the_gather(m, twin):
    n = 1501
    rng = np.random.default_rng(m)
    K = rng.normal(size=(n, n))
    pts = 2 * n if twin else n
    inner = rng.choice(np.arange(1, pts - 1), size=max(m - 2, 0), replace=False)
    W = np.sort(np.r_[[pts - 1, 0][: min(m, 2)], inner]).astype(np.int64)  # ascending, both ends of the range
    if twin:  # both points of one row
        W = np.unique(np.r_[W, 7, 7 + n])
    Wd = torch.from_numpy(W.astype(np.int32)).to(DEV)
    np.testing.assert_array_equal(D.gram_kww(_device(K), Wd).cpu().numpy(), K[np.ix_(W % n, W % n)])
    assert not D.gram_kww(_device(K), Wd, gate=1).any()  # a set gate writes nothing


@pytest.mark.parametrize("where", [None, (0, 129), (63, 64), (129, 128), "nan"])
def test_check_names_the_first_offending_entry(where):
    n = 130
    K = np.random.default_rng(3).normal(size=(n, n))
    K = (K + K.T) / 2
    want = -1
    if where == "nan":
        K[70, 70] = np.nan
        want = 70 * n + 70
    elif where:
        K.view(np.int64)[where] ^= 1  # one low bit; the pair's first entry in row-major order is reported
        want = min(where) * n + max(where)
    assert D.gram_check(_device(K)) == want
    assert D.gram_check(D.device_gram(K, DEV)) == want  # the padded upload


@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("nsv", [0, 1, 63, 64, 65, 1500])
def test_decision_gathers_the_support_columns(nsv, m):
    ncol = 1601
    rng = np.random.default_rng(nsv + m)
    Kq = rng.normal(size=(m, ncol))
    sv = np.sort(rng.choice(ncol, size=nsv, replace=False)).astype(np.int32)
    coef = rng.normal(size=nsv)
    svd, cd = torch.from_numpy(sv).to(DEV), torch.from_numpy(coef).to(DEV)
    got = D.decision_gram(Kq, svd, cd, 0.0, chunk_rows=2).cpu().numpy()  # uploaded in row chunks
    P = Kq[:, sv] * coef
    ref = np.array([math.fsum(P[q]) for q in range(m)])
    assert np.all(np.abs(got - ref) <= (nsv / 64 + 8) * U * np.abs(P).sum(1))
    # a device tensor read in place, and b: one subtraction from the same sum
    np.testing.assert_array_equal(D.decision_gram(_device(Kq), svd, cd, 0.375).cpu().numpy(), got - 0.375)
