"""The float16 RBF block (rows_f16.hip) through svmd_rbf_block_f16 against numpy float64 on the device's own float16
values: the store epilogue at the edges of a wave's 32-row slice, the workgroup's 128-row tile, the 64-column tile and
the 64-half k stage, with subnormal halves, its symmetry and id rule, and the sum epilogues' bound, determinism, twin
form and no-op cases.

Bound of the store epilogue (the float32 test's): the products of two float16 values are exact in float32, so the only
error of a dot product is its d float32 adds, gamma_d sum |a_k b_k| with gamma_d = d u / (1 - d u); u = 2^-23 is one
factor of two over round-to-nearest because the MFMA's internal adds are not documented.  exp(-gamma x) has slope at
most gamma and the distance holds 2 a.b, hence 2 gamma; 1e-14 covers the FP64 epilogue."""
import numpy as np
import pytest
import torch

from svm355.ops import device as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0**-23


def _rows(seed, n, d, scale=None):
    X = np.random.default_rng(seed).uniform(0.0, 1.0, (n, d))
    if scale is not None:
        X = X * scale
    X = X.astype(np.float32).astype(np.float16)
    return X, D.upload_rows_f16(X, DEV)


# (A rows, device-side column count, B rows, d, columns scaled by 2^-16: of B, or of A when negative): not the cross product
CASES = [(1, 1, 1, 1, 0), (31, 63, 63, 63, 0), (32, 64, 64, 64, 0), (33, 65, 65, 65, 0), (127, 1024, 1024, 17, 0),
         (128, 65, 65, 784, 0), (129, 1024, 1024, 784, 0), (129, 200, 300, 129, 0), (33, 65, 65, 16, 14), (33, 65, 65, 16, -14)]


@pytest.mark.parametrize("m,cnt,nb,d,sub", CASES)
def test_store_and_sums(m, cnt, nb, d, sub):
    gamma = 2.0 / d
    tiny = np.r_[np.full(abs(sub), 2.0**-16), np.ones(d - abs(sub))]
    A, Ad = _rows(m, m, d, tiny if sub < 0 else None)
    B, _ = _rows(1000 + nb, nb, d, tiny if sub > 0 else None)
    B[cnt:] = np.nan  # rows beyond the count are never read
    Bd = D.upload_rows_f16(B, DEV)
    K = D.rbf_block_f16(Ad, Bd, gamma, count=cnt).cpu().numpy()
    # the reference reads the device's own values back (subnormal halves included)
    a, b = Ad[:, :d].cpu().numpy().astype(np.float64), Bd[:cnt, :d].cpu().numpy().astype(np.float64)
    if sub:  # subnormal values of one operand against normal ones of the other: a flush of that operand would miss
        t = (b if sub > 0 else a)[:, :abs(sub)]  # the bound by a factor ~50; the two cases take the operands in turn
        assert np.all((t < 2.0**-14) & (t >= 0.0)) and np.count_nonzero(t) > t.shape[0]
    d2 = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T
    ref = np.exp(-gamma * np.maximum(d2, 0.0))
    gd = d * U / (1.0 - d * U)
    bound = 2.0 * gamma * gd * (np.abs(a) @ np.abs(b).T) + 1e-14
    err = np.abs(K[:, :cnt] - ref)
    print(f"store m={m} cnt={cnt} nb={nb} d={d} sub={sub}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
    assert np.all(err <= bound)
    assert np.all(K[:, cnt:] == 0.0)  # columns beyond the count are not written

    rng = np.random.default_rng(m + cnt)
    coef, f0 = rng.uniform(-10.0, 10.0, nb), rng.normal(size=2 * m)
    cd = torch.from_numpy(coef).to(DEV)

    def run(epi, count, gate=0, start=f0):
        f = torch.from_numpy(start[: m * (2 if epi == "sum_twin" else 1)].copy()).to(DEV)
        return D.rbf_block_f16(Ad, Bd, gamma, epi, coef=cd, f=f, count=count, gate=gate).cpu().numpy()

    zero = run("sum", cnt, start=np.zeros(2 * m))  # into f = 0 the add is exact: the bound is on the terms alone
    want = (K[:, :cnt].astype(np.longdouble) * coef[:cnt]).sum(1)
    sbound = (cnt + 6) * 2.0**-53 * np.abs(coef[:cnt] * K[:, :cnt]).sum(1)
    serr = np.abs(zero - want).astype(np.float64)
    print(f"sum: max err {serr.max():.3e}, max err / bound {(serr / sbound).max():.3f}")
    assert np.all(serr <= sbound)
    out = run("sum", cnt)
    np.testing.assert_array_equal(out, f0[:m] + zero)  # into a non-zero f: the same sum, one add
    np.testing.assert_array_equal(run("sum", cnt), out)  # two launches, the same bits
    tw = run("sum_twin", cnt)
    np.testing.assert_array_equal(tw[:m], out)
    np.testing.assert_array_equal(tw[m:], f0[m:] + zero)
    np.testing.assert_array_equal(run("sum_twin", 0), f0)  # a count of 0 and a non-zero gate write nothing
    np.testing.assert_array_equal(run("sum", cnt, gate=1), f0[:m])


@pytest.mark.parametrize("d", [1, 17, 784])
def test_symmetry_and_ids(d):
    n, nrow = 139, 130
    gamma = 2.0 / d
    X, Xd = _rows(d, nrow, d)
    W = np.concatenate([np.arange(nrow), nrow + np.arange(9)]).astype(np.int32)  # every row, 9 of them with both twins
    Wd = torch.from_numpy(W).to(DEV)
    G = Xd[torch.from_numpy(W % nrow).to(DEV).long()].contiguous()  # the gathered working set, as the solver's
    plain = D.rbf_block_f16(G, G, gamma)
    assert torch.equal(plain, plain.T.contiguous())
    K = D.rbf_block_f16(G, G, gamma, ida=Wd, idb=Wd, twin_nrow=nrow)
    assert torch.equal(K, K.T.contiguous())
    same = torch.from_numpy((W % nrow)[:, None] == (W % nrow)[None, :]).to(DEV)
    assert int(same.sum()) == n + 18
    assert bool((K[same] == 1.0).all()) and torch.equal(K[~same], plain[~same])
    off = D.rbf_block_f16(G[:64].contiguous(), G, gamma, idb=Wd, row_off=3)  # A row i is training row 3 + i
    hit = torch.from_numpy((3 + np.arange(64))[:, None] == W[None, :]).to(DEV)
    assert bool((off[hit] == 1.0).all()) and torch.equal(off[~hit], plain[:64][~hit])
