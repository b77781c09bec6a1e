"""One-GPU epsilon-SVR fits for profiles/svr.md, and the classification fit of the same rows next to them.

    python scripts/svr_profile.py --input pixel|real --mode svr|svc [--n 60000] [--reps 3]
    python scripts/svr_profile.py --census DIR      # summarise rocprofv3 --kernel-trace CSVs found under DIR

Inputs (both seeded, nothing read from disk):
  pixel  synthetic_mnist(n, seed=1) uint8 rows; regression target z = the row's mean intensity / 16
         (SVR: C = 10, gamma = 0.00125, epsilon = 0.05); classification labels: the generator's one-vs-rest y
  real   n x 8 uniform rows in [0, 1], z = sin(X w) + 0.05 noise (tests/svr_checks.py's generator)
         (SVR: C = 10, gamma = 0.5, epsilon = 0.1); classification labels: z above / below its median
A fit is timed by the host clock around fit() (it ends in device-to-host copies of the alphas); the first fit of
the process is reported apart (it loads code objects).  Under rocprofv3 run one mode with --reps 1.
"""
import argparse
import csv
import json
import sys
import time
from collections import defaultdict
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def rows(kind: str, n: int):
    if kind == "pixel":
        from svm355.utils.data import synthetic_mnist

        tr = synthetic_mnist(n, seed=1).compact()
        z = np.ascontiguousarray(tr.X.astype(np.float64).mean(axis=1) / 16.0)
        return tr.X, z, tr.y, dict(C=10.0, gamma=0.00125, epsilon=0.05)
    from svr_checks import real_rows

    X, z = real_rows(n, seed=1)
    return X, z, np.where(z > np.median(z), 1, -1).astype(np.int32), dict(C=10.0, gamma=0.5, epsilon=0.1)


def fit(kind: str, mode: str, n: int, reps: int) -> None:
    from svm355 import SVC, SVR

    X, z, y, hp = rows(kind, n)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        if mode == "svr":
            m = SVR(device="cuda:0", max_iter=10**8, **hp).fit(X, z)
        else:
            m = SVC(device="cuda:0", solver="decomp", C=hp["C"], gamma=hp["gamma"], max_iter=10**8).fit(X, y)
        times.append((time.perf_counter() - t0) * 1e3)
    tm = m.timings_
    out = {"input": kind, "mode": mode, "n": n, "first_fit_ms": round(times[0], 2),
           "fit_ms": [round(t, 2) for t in times[1:]], "solve_ms": round(tm["smo_ms"], 2),
           "quantise_ms": round(tm["gram_ms"], 2), "stop": m.stop_reason_, "outer_iterations": tm["outer_iterations"],
           "pair_updates": tm["inner_iterations"], "update_columns": tm["update_columns"],
           "gram_path": tm["gram_path"], "n_sv": int(len(m.support_))}
    if mode == "svr":
        pred = m.predict(X[:5000])
        out["max_abs_residual_5000"] = float(np.abs(pred - z[:5000]).max())
        out["r2_5000"] = round(m.score(X[:5000], z[:5000]), 6)
    print(json.dumps(out), flush=True)


def census(directory: str) -> None:
    """Per kernel of every *kernel_trace.csv under `directory`: launches, mean and total time, the grid sizes."""
    for path in sorted(Path(directory).rglob("*kernel_trace.csv")):
        agg = defaultdict(lambda: [0, 0, set()])
        with open(path, newline="") as fh:
            rd = csv.DictReader(fh)
            need = {"Kernel_Name", "Start_Timestamp", "End_Timestamp", "Grid_Size_X", "Workgroup_Size_X"}
            if not need <= set(rd.fieldnames or ()):
                print(f"== {path}: unexpected columns {rd.fieldnames}")
                continue
            for r in rd:
                a = agg[r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")]
                a[0] += 1
                a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
                a[2].add((int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"])))
        print(f"== {path.relative_to(directory)}")
        total = sum(v[1] for v in agg.values())
        print(f"{'kernel':58s} {'calls':>7s} {'mean us':>9s} {'total ms':>9s} {'share':>6s}  grid (threads) / workgroup")
        for name, (calls, ns, grids) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            g = sorted(grids)
            gs = ", ".join(f"{x}/{w}" for x, w in g[:4]) + (f", ... ({len(g)} shapes)" if len(g) > 4 else "")
            print(f"{name[:58]:58s} {calls:7d} {ns / calls / 1e3:9.2f} {ns / 1e6:9.2f} {100 * ns / total:5.1f}%  {gs}")
        print(f"{'all kernels':58s} {sum(v[0] for v in agg.values()):7d} {'':9s} {total / 1e6:9.2f}")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--input", choices=("pixel", "real"), default="pixel")
    ap.add_argument("--mode", choices=("svr", "svc"), default="svr")
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--census", metavar="DIR")
    a = ap.parse_args()
    if a.census:
        census(a.census)
    else:
        fit(a.input, a.mode, a.n, a.reps)


if __name__ == "__main__":
    main()
