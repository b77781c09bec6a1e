"""One SVC fit on bench.py's --input f64-real rows (MNIST-shaped synthetic pixels plus a uniform [0, 0.5) offset per
value: real-valued FP64 rows) with a chosen kernel, for profiles/dist_kernels.md: the laplacian / chi2 fit next to
the FP64-row RBF fit of the same rows.  Prints one JSON line; run it under rocprofv3 --kernel-trace --stats for the
per-kernel times.

    python scripts/dist_profile.py --kernel laplacian --gamma 0.005 [--n 60000]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from svm355 import SVC  # noqa: E402
from svm355.utils.data import synthetic_mnist  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="laplacian")
    ap.add_argument("--gamma", type=float, default=0.005)
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    tr = synthetic_mnist(a.n, seed=a.seed)
    X = tr.X + np.random.default_rng(a.seed + 7).uniform(0.0, 0.5, size=tr.X.shape)
    t0 = time.perf_counter()
    m = SVC(kernel=a.kernel, gamma=a.gamma, device="cuda:0").fit(X, tr.y)
    print(json.dumps({"kernel": a.kernel, "gamma": a.gamma, "n": a.n, "fit_s": round(time.perf_counter() - t0, 3),
                      "stop": m.stop_reason_, "n_iter": int(m.n_iter_), "n_sv": int(len(m.support_)),
                      "timings": {k: v for k, v in m.timings_.items() if isinstance(v, (int, float, str))}}))


if __name__ == "__main__":
    main()
