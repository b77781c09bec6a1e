"""Measurements for profiles/precomputed.md on one GPU.  Rows: bench.py's --input f64-real shape (MNIST-shaped
synthetic pixels plus a uniform [0, 0.5) offset per value), min-max scaled; the Gram is their linear Gram, built and
symmetrised on the device.

    python scripts/precomputed_profile.py rowsum [--n 60000] [--moved 1024] [--reps 50]
        the f update alone: gram_rowsum_kernel on `moved` rows of the Gram next to the linear kernel's fused block and
        sum (kfun_block_kernel) on the rows that produced it, `reps` launches each.  Run it under rocprofv3
        --kernel-trace --stats for the kernel times; it prints the bytes the row sum must move, n x moved x 8.
    python scripts/precomputed_profile.py fit [--n 60000] [--max-iter 20000]
        SVC(kernel="precomputed").fit on the device Gram next to SVC(kernel="linear").fit on the rows, both capped at
        the same number of pair updates.  Prints one JSON line each.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from svm355 import SVC, SVMParams  # noqa: E402
from svm355.ops import device as D  # noqa: E402
from svm355.utils.data import synthetic_mnist  # noqa: E402

DEV = torch.device("cuda:0")


def rows(n: int, seed: int):
    tr = synthetic_mnist(n, seed=seed)
    X = tr.X + np.random.default_rng(seed + 7).uniform(0.0, 0.5, size=tr.X.shape)
    return X, tr.y


def device_rows_and_gram(X):
    """The scaled, padded device rows and their linear Gram, symmetric to the bit, in device_gram's form."""
    r = D.upload_rows(X, DEV)
    D.minmax_scale_(r, X.shape[1])
    n = r.shape[0]
    K = torch.empty((n, D.padded_gram_dim(n)), dtype=torch.float64, device=DEV)[:, :n]
    G = r @ r.T
    step = 4096
    for i in range(0, n, step):  # (G + G') / 2 of one G, block by block: the addition commutes, so K = K' to the bit
        K[i:i + step] = (G[i:i + step] + G[:, i:i + step].T) / 2
    del G
    torch.cuda.synchronize()
    return r, K


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["rowsum", "fit"])
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--moved", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    X, y = rows(a.n, a.seed)
    r, K = device_rows_and_gram(X)
    assert D.gram_check(K) == -1
    if a.what == "rowsum":
        rng = np.random.default_rng(3)
        cols = torch.from_numpy(np.sort(rng.choice(a.n, a.moved, replace=False)).astype(np.int32)).to(DEV)
        coef = torch.from_numpy(rng.normal(size=a.moved)).to(DEV)
        f = torch.zeros(a.n, dtype=torch.float64, device=DEV)
        B = r[cols.long()].contiguous()
        p = SVMParams(kernel="linear")
        out = {}
        for name, fn in (("gram_rowsum", lambda: D.gram_rowsum(K, cols, coef, f, a.moved)),
                         ("kfun_block_sum", lambda: D.kfun_block(r, B, p, "sum", coef=coef, f=f, count=a.moved))):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()  # each call ends in a stream synchronise
            out[name + "_call_ms"] = round((time.perf_counter() - t0) / a.reps * 1e3, 4)
        print(json.dumps({"n": a.n, "moved": a.moved, "reps": a.reps, "ld": K.stride(0),
                          "rowsum_bytes": a.n * a.moved * 8, **out}))
        return
    for kernel, data in (("precomputed", K), ("linear", X), ("precomputed", K), ("linear", X)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = SVC(kernel=kernel, max_iter=a.max_iter, device="cuda:0").fit(data, y)
        torch.cuda.synchronize()
        print(json.dumps({"kernel": kernel, "n": a.n, "fit_s": round(time.perf_counter() - t0, 4), "stop": m.stop_reason_,
                          "n_iter": int(m.n_iter_), "n_sv": int(len(m.support_)),
                          "timings": {k: v for k, v in m.timings_.items() if isinstance(v, (int, float, str))}}))


if __name__ == "__main__":
    main()
