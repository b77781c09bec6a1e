"""The linear kernel on CSR rows (csr_linear.hip) against numpy longdouble on the densified rows: the dot block, the
f update as the solver runs it (panel scatter, panel reduce, CSR x vector) and the weight vector with the decision
function of CSR queries.  Rows are test_gpu_csr_kernel.py's: lengths cycle through {129, 0, 1, 63, 64, 65} (the
64-pair fetch edge and an empty row), row 0 uses features 0 and d - 1, values in (0, 1].

Bounds (derived, for any summation order; u = 2^-53).  Block: kernel_ref's (d + 2) u sum |a||b| -- a row stores at
most d values and absent features add exact zeros.  f update: a term coef_j B_jc a_ic of f_i passes at most cnt
roundings in dw (its product and the adds of the cnt-term sum), at most z_i (row i's stored count) in the product
with a_i, then one add into f_i, relative to the result; with the reference's own rounding and the second-order
terms in the slack of 4,  |f - ref|_i <= (cnt + z_i + 4) u S_i + u |ref_i|,  S_i = sum_c |a_ic| sum_j |coef_j| |B_jc|.
Decision: the same with nsv for cnt, and |b| beside |ref_i| (out starts at -b).
"""
import numpy as np
import pytest
import torch

from kfun_checks import U, kernel_ref
from test_gpu_csr_kernel import device_rows, make_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LD = np.longdouble


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sum_ref(A, B, coef, base, terms):
    """(ref, bound) of base + A (B' coef) in longdouble, `terms` = B's rows (cnt or nsv)."""
    ref = base.astype(LD) + A.astype(LD) @ (coef.astype(LD) @ B.astype(LD))
    S = np.abs(A) @ (np.abs(coef) @ np.abs(B))
    return ref.astype(np.float64), (terms + (A != 0).sum(1) + 4) * U * S + U * np.abs(ref).astype(np.float64)


@pytest.mark.parametrize("nb,m,d", [(1, 1, 1), (63, 4, 17), (64, 5, 4099), (65, 9, 17), (1024, 5, 17)])
def test_block_matches_longdouble(nb, m, d):
    from svm355.ops import device as D

    rng = np.random.default_rng(1000 * nb + m)
    (Xa, A), (Xb, B) = make_rows(rng, m, d), make_rows(rng, nb, d)
    Rb = device_rows(D, Xb)
    K = D.linear_block_csr(device_rows(D, Xa), Rb).cpu().numpy()
    ref, bound = kernel_ref(A, B, "linear")
    print(f"block nb={nb} m={m} d={d}: max |K - ref| = {np.abs(K - ref).max():.3e} (bound {bound.max():.3e})")
    assert np.all(np.abs(K - ref) <= bound)
    if nb == 65:  # sorted indices, no contraction, exact zeros: symmetric to the bit
        Krr = D.linear_block_csr(Rb, Rb).cpu().numpy()
        assert np.array_equal(Krr, Krr.T)


@pytest.mark.parametrize("cnt,m,d,twin", [(1, 1, 17, False), (64, 5, 4099, False), (65, 9, 17, True),
                                          (1024, 5, 17, False), (1024, 9, 4099, True)])
def test_f_update_matches_longdouble(cnt, m, d, twin):
    from svm355.ops import device as D

    rng = np.random.default_rng(77 * cnt + m)
    (Xa, A), (Xb, B) = make_rows(rng, m, d), make_rows(rng, cnt, d)
    Ra, Rb = device_rows(D, Xa), device_rows(D, Xb)
    coef, f0 = rng.normal(size=cnt), rng.normal(size=m * (2 if twin else 1))
    f = D.linear_fupdate_csr(Ra, Rb, dev(coef), dev(f0), twin=twin)
    again = D.linear_fupdate_csr(Ra, Rb, dev(coef), dev(f0), twin=twin)
    assert torch.equal(f, again)  # a fixed summation order: the same bits on every run
    reps = 2 if twin else 1
    ref, bound = sum_ref(np.tile(A, (reps, 1)), B, coef, f0, cnt)
    err = np.abs(f.cpu().numpy() - ref)
    print(f"f update cnt={cnt} m={m} d={d} twin={twin}: max |f - ref| = {err.max():.3e}, "
          f"largest share of the bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)
    kept = D.linear_fupdate_csr(Ra, Rb, dev(coef), dev(f0), twin=twin, count=0)
    assert np.array_equal(kept.cpu().numpy().view(np.int64), f0.view(np.int64))  # a device count of 0


@pytest.mark.parametrize("nsv,m,d", [(1, 1, 4099), (1024, 5, 17), (1025, 5, 4099), (2049, 1, 17)])
def test_weight_vector_and_decision_match_longdouble(nsv, m, d):
    from svm355.ops import device as D

    rng = np.random.default_rng(13 * nsv + m)
    Xq, Q = make_rows(rng, m, d)
    Xs = rng.random((nsv, d)) * (rng.random((nsv, d)) < 0.3)
    coef, b = rng.normal(size=nsv), 0.75
    w = D.linear_w(D.upload_rows(Xs, torch.device(DEV)), dev(coef))
    wref = (coef.astype(LD) @ Xs.astype(LD)).astype(np.float64)
    werr = np.abs(w.cpu().numpy()[:d] - wref)
    assert np.all(werr <= (nsv + 2) * U * (np.abs(coef) @ Xs)) and np.all(w.cpu().numpy()[d:] == 0.0)
    out = D.decision_csr_linear(w, device_rows(D, Xq), b).cpu().numpy()
    ref, bound = sum_ref(Q, Xs, coef, np.full(m, -b), nsv)
    print(f"decision nsv={nsv} m={m} d={d}: max |w - ref| = {werr.max():.3e}, max |out - ref| = "
          f"{np.abs(out - ref).max():.3e} (bound {bound.max() + U * b:.3e})")
    assert np.all(np.abs(out - ref) <= bound + U * abs(b))
