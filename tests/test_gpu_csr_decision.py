"""svmd_decision_csr: CSR queries against dense support vectors -- the LDS tile transpose of each chunk of 1024
support vectors into the panel, and the sum epilogue of the CSR x panel kernel -- against numpy.

nsv at the chunk edges (1, 1024, 1025, 2049), m = 1 and 5 queries (one wave, and a second workgroup), d = 40 with
at most 32 nonzeros per query, coefficients in [-1, 1].  atol = nsv x 2e-12: the per-value bound at nnz <= 32
((32 + 3) 2^-53 x 4 x 32 x gamma, under 1e-12 at gamma = 0.5) times the number of terms; rtol = 0.  Two runs give
the same bits (the sum's order is fixed).
"""
import numpy as np
import pytest
import torch

import svm355

pytestmark = pytest.mark.gpu

D_FEAT, GAMMA, B0 = 40, 0.5, 0.25


@pytest.mark.parametrize("nsv,m", [(1, 1), (1024, 5), (1025, 1), (2049, 5)])
def test_decision_matches_numpy(nsv, m):
    from svm355.ops import device as D

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(nsv + m)
    S = rng.random((nsv, D_FEAT)) * (rng.random((nsv, D_FEAT)) < 0.3)
    Q = np.zeros((m, D_FEAT))
    for i in range(m):
        idx = rng.choice(D_FEAT, [32, 0, 1, 17, 5][i], replace=False)
        Q[i, idx] = 1.0 - rng.random(len(idx))
    coef = rng.uniform(-1.0, 1.0, nsv)
    Xs = D.upload_rows(S, dev)
    ns = D.row_norms(Xs, D_FEAT)
    Qd = D.upload_csr(svm355.CSR.from_dense(Q), dev)
    D.csr_prepare(Qd, scale=False)
    coef_d = torch.from_numpy(coef).to(dev)
    out = D.decision_csr(Xs, ns, coef_d, Qd, GAMMA, B0).cpu().numpy()
    again = D.decision_csr(Xs, ns, coef_d, Qd, GAMMA, B0).cpu().numpy()
    d2 = (Q * Q).sum(1)[:, None] + (S * S).sum(1)[None, :] - 2.0 * Q @ S.T
    ref = np.exp(-GAMMA * np.maximum(d2, 0.0)) @ coef - B0
    print(f"nsv={nsv} m={m}: max |out - ref| = {np.abs(out - ref).max():.3e}")
    np.testing.assert_allclose(out, ref, rtol=0, atol=nsv * 2e-12)
    assert np.array_equal(out, again)
