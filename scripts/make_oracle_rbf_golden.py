"""Writes tests/golden/oracle_rbf_n128.npz: the decomposition oracle's RBF outputs (svm_decomp_train_gram_rows,
svm_decomp_train_gram_svr) on one small case, recorded on the commit BEFORE svm_params gained its kernel fields.
tests/test_kfun_cpu.py asserts that the oracle with kernel == 0 still returns these bits: the kernel fields may
not change one operation of the RBF arithmetic.  Run it only on that commit; on a later one it would record what
it is meant to check.

Case: 128 x 8 real-valued rows (tests/svr_checks.py real_rows, seed 5), the RBF Gram at gamma = 0.5 (stored, so
no exp is recomputed), labels by the targets' median, C = 10.  Three solves (working set 1024, 64, 64): the classifier with
inner_wss = 3 in the exact-integer GEMV's order, with inner_wss = 2 in the FP64-row order, and the twin
(epsilon-SVR) mode with inner_wss = 3 in the FP64-row order.

    python scripts/make_oracle_rbf_golden.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))


def solves(K, y, z):
    """{name: (alpha, b, iterations)} of the three oracle solves (shared with the test)."""
    from svm355 import SVMParams
    from svm355.ops import cpu as C

    p = SVMParams(C=10.0, gamma=0.5, n_threads=1)
    out = {}
    a, r, _, _ = C.decomp_train_gram(K, y, p, q=1024, inner_wss=3)
    out["svc3"] = (a, r.b, r.iterations)
    a, r, _, _ = C.decomp_train_gram(K, y, p, q=64, inner_wss=2, fp64_rows=True)
    out["svc2"] = (a, r.b, r.iterations)
    a, r, _, _ = C.decomp_train_gram_svr(K, z, p, 0.1, q=64, inner_wss=3, fp64_rows=True)
    out["svr3"] = (a, r.b, r.iterations)
    return out


def main() -> None:
    from svr_checks import rbf_numpy, real_rows

    X, z = real_rows(128, 5)
    K = np.ascontiguousarray(rbf_numpy(X, X, 0.5))
    y = np.where(z > np.median(z), 1, -1).astype(np.int32)
    rec = {"K": K, "y": y, "z": z}
    for name, (a, b, it) in solves(K, y, z).items():
        rec.update({f"{name}_alpha": a, f"{name}_b": np.array(b), f"{name}_iterations": np.array(it)})
        print(name, "iterations", it, "b", b)
    dst = ROOT / "tests" / "golden" / "oracle_rbf_n128.npz"
    np.savez_compressed(dst, **rec)
    print(dst, dst.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
