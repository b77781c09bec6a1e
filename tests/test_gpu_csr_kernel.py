"""svmd_rbf_block_csr (csr_rbf.hip: the panel scatter and the store kernel) against numpy on the densified rows.

Shapes: panel rows nb at the lane and accumulator edges (1, 63, 64, 65, 1023, 1024), CSR rows m around the
workgroup's 4 waves (1, 4, 5, 9), d in {1, 17, 4099}, row lengths from {0, 1, 63, 64, 65, 129} (the 64-pair fetch
edge; capped at d).  Every side of two or more rows holds an empty row and a row that uses feature 0 and feature
d - 1; a side of one row holds the latter.  Values are in (0, 1].

Tolerance (derived, not fitted): with nnz <= 129 and values <= 1 the rounding of |a|^2 + |b|^2 - 2 a.b is at most
(nnz + 3) 2^-53 (|a|^2 + |b|^2 + 2 sum |a||b|) <= 132 x 1.1e-16 x 516 ~ 7.5e-12, and K's error at most gamma
times that plus a few ulp: atol = 1e-11, rtol = 0.
"""
import numpy as np
import pytest
import torch

import svm355

pytestmark = pytest.mark.gpu

LENS = (129, 0, 1, 63, 64, 65)
ATOL = 1e-11


def make_rows(rng, m, d):
    """m rows of d features as (svm355.CSR, dense): lengths cycle through LENS, row 0 uses features 0 and d - 1."""
    dense = np.zeros((m, d))
    for i in range(m):
        idx = np.sort(rng.choice(d, min(LENS[i % len(LENS)], d), replace=False))
        if i == 0:
            idx[0], idx[-1] = 0, d - 1
        dense[i, idx] = 1.0 - rng.random(len(idx))
    return svm355.CSR.from_dense(dense), dense


def device_rows(D, X):
    A = D.upload_csr(X, torch.device("cuda:0"))
    D.csr_prepare(A, scale=False)
    return A


def rbf_ref(A, B, gamma):
    d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A @ B.T
    return np.exp(-gamma * np.maximum(d2, 0.0))


@pytest.mark.parametrize("nb,m,d,gamma", [(1, 1, 1, 0.5), (63, 4, 17, 0.00125), (64, 5, 4099, 0.5), (65, 9, 17, 0.5),
                                          (1023, 4, 4099, 0.00125), (1024, 5, 17, 0.5), (1024, 9, 1, 0.00125)])
def test_block_matches_numpy(nb, m, d, gamma):
    from svm355.ops import device as D

    rng = np.random.default_rng(1000 * nb + m)
    (Xa, A), (Xb, B) = make_rows(rng, m, d), make_rows(rng, nb, d)
    K = D.rbf_block_csr(device_rows(D, Xa), device_rows(D, Xb), gamma).cpu().numpy()
    ref = rbf_ref(A, B, gamma)
    print(f"nb={nb} m={m} d={d} gamma={gamma}: max |K - ref| = {np.abs(K - ref).max():.3e}")
    np.testing.assert_allclose(K, ref, rtol=0, atol=ATOL)


def test_same_training_row_is_exactly_one():
    from svm355.ops import device as D

    rng = np.random.default_rng(7)
    X, A = make_rows(rng, 65, 4099)
    R = device_rows(D, X)
    ids = torch.arange(7, 72, dtype=torch.int32, device="cuda:0")  # panel row j is training row 7 + j
    K = D.rbf_block_csr(R, R, 0.5, ids=ids, row_off=7).cpu().numpy()
    assert np.all(np.diag(K) == 1.0) and K.max() <= 1.0
    np.testing.assert_allclose(K, rbf_ref(A, A, 0.5), rtol=0, atol=ATOL)
