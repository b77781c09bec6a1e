"""The dot-product kernel block (decomp_kfun.hip) through svmd_kfun_block against a longdouble numpy reference: the
store epilogue at the edges of its 64 x 64 tiles and of its 16-double k stage, its symmetry to the bit, and the sum
epilogues' bounds, no-op cases, determinism and twin form."""
import numpy as np
import pytest
import torch

from svm355 import SVMParams
from svm355.ops import device as D

from kfun_checks import TANH_DEV, U, kernel_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _cases(d):
    return {"linear": dict(kernel="linear"), "poly3": dict(kernel="poly", degree=3, gamma=0.5, coef0=1.0),
            "poly1": dict(kernel="poly", degree=1, gamma=1.0, coef0=0.0),
            "sigmoid": dict(kernel="sigmoid", gamma=1.0 / d, coef0=-1.0)}


def _bound(kw, bound):
    return bound + (4 * TANH_DEV if kw["kernel"] == "sigmoid" else 0.0)


@pytest.mark.parametrize("d", [1, 15, 16, 17, 40])
@pytest.mark.parametrize("name", ["linear", "poly3", "poly1", "sigmoid"])
def test_store_against_longdouble_and_symmetry(name, d):
    kw = _cases(d)[name]
    p = SVMParams(**{"gamma": 1.0, **kw})
    rng = np.random.default_rng(100 * d + len(name))
    X = rng.uniform(0.0, 1.0, (257, d))
    Xd = D.upload_rows(X, DEV)
    for m, n in [(1, 1), (63, 65), (64, 64), (65, 63), (129, 257), (257, 129)]:
        K = D.kfun_block(Xd[:m].contiguous(), Xd[:n].contiguous(), p).cpu().numpy()
        ref, bound = kernel_ref(X[:m], X[:n], **{"gamma": 1.0, **kw})
        err = np.abs(K - ref)
        print(f"{name} d={d} m={m} n={n}: max err {err.max():.3e}, max err - bound {(err - bound).max():.3e}")
        assert np.all(err <= _bound(kw, bound)), (name, d, m, n)
    K = D.kfun_block(Xd, Xd, p)
    assert torch.equal(K, K.T.contiguous())


@pytest.mark.parametrize("n", [1, 129, 300])
@pytest.mark.parametrize("name", ["linear", "poly3", "sigmoid"])
def test_sum_epilogues(name, n):
    d = 17
    kw = _cases(d)[name]
    p = SVMParams(**{"gamma": 1.0, **kw})
    rng = np.random.default_rng(n + len(name))
    X, B = rng.uniform(0.0, 1.0, (n, d)), rng.uniform(0.0, 1.0, (1024, d))
    coef, f0 = rng.uniform(-10.0, 10.0, 1024), rng.normal(size=2 * n)
    Xd, Bd, cd = D.upload_rows(X, DEV), D.upload_rows(B, DEV), torch.from_numpy(coef).to(DEV)
    ref, kb = kernel_ref(X, B, **{"gamma": 1.0, **kw})
    kb = _bound(kw, kb)

    def run(epi, cnt, gate=0, start=None):
        f = torch.from_numpy((f0[: n * (2 if epi == "sum_twin" else 1)] if start is None else start).copy()).to(DEV)
        return D.kfun_block(Xd, Bd, p, epi, coef=cd, f=f, count=cnt, gate=gate).cpu().numpy()

    for cnt in (0, 1, 127, 128, 129, 1024):
        out = run("sum", cnt)
        if cnt == 0:
            np.testing.assert_array_equal(out, f0[:n])
            continue
        # the issue's bound, asserted on a sum into f = 0 (the add into f is then exact; a non-zero f would round once
        # more, by u |f|, which the bound -- relative to the terms alone -- does not hold), against the reference's
        # sum formed in longdouble
        zero = run("sum", cnt, start=np.zeros(n))
        want = ref[:, :cnt].astype(np.longdouble) @ coef[:cnt]
        bound = (cnt + d + 4) * U * np.abs(coef[:cnt] * ref[:, :cnt]).sum(1) + kb[:, :cnt] @ np.abs(coef[:cnt])
        err = np.abs(zero - want).astype(np.float64)
        print(f"{name} n={n} cnt={cnt}: max (err - bound) {(err - bound).max():.3e}, max err {err.max():.3e}")
        assert np.all(err <= bound), (name, n, cnt)
        np.testing.assert_array_equal(out, f0[:n] + zero)  # into a non-zero f: the same sum, one add
        np.testing.assert_array_equal(run("sum", cnt), out)  # two runs, the same bits
        tw = run("sum_twin", cnt)  # the same sum into f[k] and f[k + n]: the plain form from each half's start
        np.testing.assert_array_equal(tw[:n], out)
        np.testing.assert_array_equal(tw[n:], run("sum", cnt, start=f0[n:]))
    np.testing.assert_array_equal(run("sum", 129, gate=1), f0[:n])  # a stopped solve's launch is a no-op
