"""The float32 RBF block (rows_f32.hip) through svmd_rbf_block_f32 against numpy float64 on the same float32 values:
the store epilogue at the edges of a wave's 32-row slice, the workgroup's 128-row tile, the 64-column tile and the
16-float k stage, its symmetry and id rule, and the sum epilogues' bound, determinism, twin form and no-op cases."""
import numpy as np
import pytest
import torch

from svm355.ops import device as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0**-23  # the derivation under round-to-nearest has 2^-24; the MFMA's internal adds are not documented


def _rows(seed, n, d):
    X = np.random.default_rng(seed).uniform(0.0, 1.0, (n, d)).astype(np.float32)
    return X, D.upload_rows_f32(X, DEV)


# (A rows, device-side column count, B rows, d): not the cross product
CASES = [(1, 1, 1, 1), (31, 63, 63, 17), (32, 64, 64, 17), (33, 65, 65, 1), (127, 1024, 1024, 17), (128, 65, 65, 784),
         (129, 1024, 1024, 784), (129, 200, 300, 17)]


@pytest.mark.parametrize("m,cnt,nb,d", CASES)
def test_store_and_sums(m, cnt, nb, d):
    gamma = 2.0 / d
    A, Ad = _rows(m, m, d)
    B, _ = _rows(1000 + nb, nb, d)
    B[cnt:] = np.nan  # rows beyond the count are never read
    Bd = D.upload_rows_f32(B, DEV)
    K = D.rbf_block_f32(Ad, Bd, gamma, count=cnt).cpu().numpy()
    a, b = A.astype(np.float64), B[:cnt].astype(np.float64)
    d2 = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T
    ref = np.exp(-gamma * np.maximum(d2, 0.0))
    gd = d * U / (1.0 - d * U)
    bound = 2.0 * gamma * gd * (np.abs(a) @ np.abs(b).T) + 1e-14
    err = np.abs(K[:, :cnt] - ref)
    print(f"store m={m} cnt={cnt} nb={nb} d={d}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
    assert np.all(err <= bound)
    assert np.all(K[:, cnt:] == 0.0)  # columns beyond the count are not written

    rng = np.random.default_rng(m + cnt)
    coef, f0 = rng.uniform(-10.0, 10.0, nb), rng.normal(size=2 * m)
    cd = torch.from_numpy(coef).to(DEV)

    def run(epi, count, gate=0, start=f0):
        f = torch.from_numpy(start[: m * (2 if epi == "sum_twin" else 1)].copy()).to(DEV)
        return D.rbf_block_f32(Ad, Bd, gamma, epi, coef=cd, f=f, count=count, gate=gate).cpu().numpy()

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
    plain = D.rbf_block_f32(G, G, gamma)
    assert torch.equal(plain, plain.T.contiguous())
    K = D.rbf_block_f32(G, G, gamma, ida=Wd, idb=Wd, twin_nrow=nrow)
    assert torch.equal(K, K.T.contiguous())
    same = torch.from_numpy((W % nrow)[:, None] == (W % nrow)[None, :]).to(DEV)
    assert int(same.sum()) == n + 18
    assert bool((K[same] == 1.0).all()) and torch.equal(K[~same], plain[~same])
    off = D.rbf_block_f32(G[:64].contiguous(), G, gamma, idb=Wd, row_off=3)  # A row i is training row 3 + i
    hit = torch.from_numpy((3 + np.arange(64))[:, None] == W[None, :]).to(DEV)
    assert bool((off[hit] == 1.0).all()) and torch.equal(off[~hit], plain[:64][~hit])
