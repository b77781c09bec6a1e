"""The one-vs-one vote kernel (csrc/hip/ovo.hip: svmd_ovo_votes, svmd_ovo_predict) against its host twin
``ops.cpu.ovo_votes`` in FP64, at the shapes where its loops can go wrong: the accumulator group of 8 splits at
k - 1 = 8 | 9 | 16, the four waves loop over more than four classes from k = 5, segments of 0 (first, middle and
last), 1, 63, 64, 65 and 129 support vectors, 1 / 3 / 130 query rows (a workgroup takes four: 130 leaves two),
k = 32 | 33 where it goes back to one row per workgroup, k = 64, pad columns full of NaN in K and coef.

Tolerance (derived, ovo_checks.vote_bound): two FP64 summations of a pair's n_a + n_b terms in different orders
are at most 2 (n_a + n_b + 2) 2^-53 (sum |coef K| + |rho|) apart."""
import numpy as np
import pytest
import torch

from svm355.ops import cpu as C
from svm355.ops import device as D

from ovo_checks import exact_case, pairs, tie_wins, vote_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# k, segment lengths, query rows
SHAPES = [
    (2, [63, 64], 1),
    (3, [0, 65, 1], 3),
    (5, [1, 0, 129, 64, 63], 130),
    (9, [3, 1, 0, 65, 2, 64, 1, 63, 5], 3),
    (10, [129, 7, 1, 64, 0, 65, 63, 2, 5, 0], 130),
    (17, [0, 5, 1, 64, 3, 65, 2, 63, 4, 1, 129, 6, 1, 2, 3, 1, 7], 3),
    # four query rows per workgroup up to k = 32, one above: both sides of the switch, and the largest k
    (32, [(7 * c) % 5 for c in range(32)], 6),
    (33, [(7 * c) % 5 for c in range(33)], 6),
    (64, [(5 * c) % 4 for c in range(64)], 3),
]


def _case(k, seg, m, seed):
    """Host (K, start, coef, rho): K uniform in (0, 1] with a NaN pad (ldk = S + 1 for odd S, S + 2 otherwise), coef
    standard normal with two NaN pad columns (ldc = S + 2)."""
    g = torch.Generator().manual_seed(seed)
    start = np.concatenate([[0], np.cumsum(seg)]).astype(np.int32)
    S = int(start[-1])
    K = np.full((m, S + (1 if S % 2 else 2)), np.nan)
    K[:, :S] = (1.0 - torch.rand((m, S), generator=g, dtype=torch.float64)).numpy()
    coef = np.full((k - 1, S + 2), np.nan)
    coef[:, :S] = torch.randn((k - 1, S), generator=g, dtype=torch.float64).numpy()
    rho = torch.randn(k * (k - 1) // 2, generator=g, dtype=torch.float64).numpy()
    return K, start, coef, rho


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


@pytest.mark.parametrize("k, seg, m", SHAPES, ids=lambda v: str(v) if isinstance(v, int) else f"S{sum(v)}")
def test_votes_against_host_twin(k, seg, m):
    K, start, coef, rho = _case(k, seg, m, seed=100 + k)
    S = int(start[-1])
    ref, rlab = C.ovo_votes(K[:, :S], start, coef[:, :S], rho)
    bound = vote_bound(K[:, :S], start, coef[:, :S], rho)
    assert np.all(np.abs(ref) > bound), "a reference decision within the bound of zero: choose another seed"
    Kd, sd, cd, rd = _dev(K, start, coef, rho)
    dec, lab = D.ovo_votes(Kd, sd, cd, rd, nsv=S)
    dec, lab = dec.cpu().numpy(), lab.cpu().numpy()
    assert dec.shape == ref.shape and lab.dtype == np.int32 and np.isfinite(dec).all()
    err = np.abs(dec - ref)
    print(f"k={k} S={S} m={m}: max |dev - ref| = {err.max():.3e}, smallest bound {bound.min():.3e}")
    assert np.all(err <= bound), float((err - bound).max())
    np.testing.assert_array_equal(lab, rlab)   # no row is excluded: every |ref| exceeds the bound
    # the labels alone (dec_d = NULL), and the same bits on a second call
    none, lab2 = D.ovo_votes(Kd, sd, cd, rd, want_dec=False, nsv=S)
    assert none is None
    np.testing.assert_array_equal(lab2.cpu().numpy(), lab)
    dec3, lab3 = D.ovo_votes(Kd, sd, cd, rd, nsv=S)
    assert torch.equal(dec3.cpu(), torch.from_numpy(dec)) and torch.equal(lab3.cpu(), torch.from_numpy(lab))


def test_empty_segments_add_exact_zero():
    """Every class empty but two: the other pairs' decisions are exactly -rho."""
    k, seg = 5, [0, 64, 0, 65, 0]
    K, start, coef, rho = _case(k, seg, 3, seed=7)
    dec, _ = D.ovo_votes(*_dev(K, start, coef, rho), nsv=int(start[-1]))
    dec = dec.cpu().numpy()
    for p, (a, b) in enumerate(pairs(k)):
        if seg[a] == 0 and seg[b] == 0:
            np.testing.assert_array_equal(dec[:, p], np.full(3, -rho[p]))


def _votes_exact(k, wins, zero=False):
    K, start, coef, rho = exact_case(k, wins)
    if zero:
        coef[:] = 0.0
    dec, lab = D.ovo_votes(*_dev(K, start.astype(np.int32), coef, rho), nsv=k)
    return dec.cpu().numpy(), lab.cpu().numpy()


def test_vote_rules():
    """Constructed inputs with exact arithmetic (K = 1, integer coefficients)."""
    dec, lab = _votes_exact(3, {(0, 1), (1, 2)})        # 0 beats 1, 1 beats 2, 2 beats 0: one vote each
    np.testing.assert_array_equal(dec, [[1.0, -1.0, 1.0]])
    assert lab[0] == 0
    dec, lab = _votes_exact(2, set(), zero=True)         # exactly 0.0 votes for b
    assert dec[0, 0] == 0.0 and not np.signbit(dec[0, 0]) and lab[0] == 1
    dec, lab = _votes_exact(10, tie_wins())              # 3 and 7 tie for the most votes: the lower index
    votes = np.zeros(10, dtype=int)
    for p, (a, b) in enumerate(pairs(10)):
        votes[a if dec[0, p] > 0 else b] += 1
    assert votes[3] == votes[7] == votes.max() and (votes == votes.max()).sum() == 2
    assert lab[0] == 3


def test_votes_refuse_bad_arguments():
    K, start, coef, rho = _case(3, [2, 2, 2], 2, seed=1)
    Kd, sd, cd, rd = _dev(K, start, coef, rho)
    with pytest.raises(ValueError):
        D.ovo_votes(Kd, sd, cd, rd[:2].contiguous(), nsv=6)           # rho of the wrong length
    with pytest.raises(ValueError):
        D.ovo_votes(Kd, sd, cd[:, :4].contiguous(), rd, nsv=6)        # coef narrower than the support vectors
    with pytest.raises(ValueError):
        D.ovo_votes(Kd, sd.to(torch.int64), cd, rd, nsv=6)            # start must be int32
    with pytest.raises(ValueError):
        D.ovo_votes(Kd, torch.zeros(67, dtype=torch.int32, device=DEV), cd, rd, nsv=0)  # 66 classes


# ------------------------------------------------------------------ svmd_ovo_predict
def _predict_case(nsv_seg, m=257, d=16, seed=3):
    r = np.random.default_rng(seed)
    k = len(nsv_seg)
    start = np.concatenate([[0], np.cumsum(nsv_seg)]).astype(np.int32)
    S = int(start[-1])
    Xs = D.upload_rows(r.uniform(size=(S, d)), DEV) if S else torch.empty((0, d), dtype=torch.float64, device=DEV)
    Xq = D.upload_rows(r.uniform(size=(m, d)), DEV)
    ns = D.row_norms(Xs, d) if S else torch.empty(0, dtype=torch.float64, device=DEV)
    nq = D.row_norms(Xq, d)
    coef, rho = r.normal(size=(k - 1, S)), r.normal(size=k * (k - 1) // 2)
    sd, cd, rd = _dev(start, coef, rho)
    return Xs, ns, Xq, nq, sd, cd, rd, (start, coef, rho)


def test_predict_chunks_and_composition():
    """m = 257 with max_rows = 128: chunks of 128, 128 and 1 rows equal the single chunk and the composition of
    rbf_gram and ovo_votes, bit for bit."""
    Xs, ns, Xq, nq, sd, cd, rd, _ = _predict_case([20, 0, 37, 13])
    gamma = 0.5
    dec1, lab1 = D.ovo_predict(Xs, ns, Xq, nq, gamma, sd, cd, rd)
    dec3, lab3 = D.ovo_predict(Xs, ns, Xq, nq, gamma, sd, cd, rd, max_rows=128)
    assert torch.equal(dec1, dec3) and torch.equal(lab1, lab3)
    dec2, lab2 = D.ovo_predict(Xs, ns, Xq, nq, gamma, sd, cd, rd, max_rows=100)  # rounded up to 128
    assert torch.equal(dec1, dec2) and torch.equal(lab1, lab2)
    Kq = D.rbf_gram(Xq, nq, Xs, ns, gamma)
    decc, labc = D.ovo_votes(Kq, sd, cd, rd, nsv=Xs.shape[0])
    assert torch.equal(dec1, decc) and torch.equal(lab1, labc)
    none, lab4 = D.ovo_predict(Xs, ns, Xq, nq, gamma, sd, cd, rd, want_dec=False, max_rows=128)
    assert none is None and torch.equal(lab1, lab4)
    assert dec1.shape == (257, 6) and torch.isfinite(dec1).all()


def test_predict_without_support_vectors():
    """nsv = 0: dec = -rho and the votes that follow from it."""
    Xs, ns, Xq, nq, sd, cd, rd, (start, coef, rho) = _predict_case([0, 0, 0, 0], m=130)
    dec, lab = D.ovo_predict(Xs, ns, Xq, nq, 0.5, sd, cd, rd, max_rows=128)
    np.testing.assert_array_equal(dec.cpu().numpy(), np.tile(-rho, (130, 1)))
    _, rlab = C.ovo_votes(np.zeros((1, 0)), start, coef, rho)
    np.testing.assert_array_equal(lab.cpu().numpy(), np.full(130, rlab[0]))
