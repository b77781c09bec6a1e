"""Measurements behind profiles/ovo.md (one GPU): the one-vs-one fit against the one-vs-rest decomposition fit on
synthetic MNIST-shaped data in one process, the width of the pair pool, and where a 10k-row one-vs-one
prediction spends its time -- the cross-kernel block, the segmented vote kernel (csrc/hip/ovo.hip), and as a
baseline the same block through torch.matmul with the dense S x P coefficient matrix plus a vote in torch.

    python scripts/ovo_profile.py [--n 60000] [--m 10000] [--part fit|predict|all] [--out ovo_profile.json]

Fits are timed by the host clock around fit() (which ends in a device synchronise), alternating the variants,
`--reps` times each after one warm-up fit of each; kernels by device events over `--kreps` launches after 3.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from svm355 import OneVsOneSVC, OneVsRestSVC  # noqa: E402
from svm355.ops import device as D  # noqa: E402
from svm355.utils.data import synthetic_mnist  # noqa: E402


def _events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def fit_part(tr, te, reps, out):
    X, Xt = tr.compact().X, te.compact().X
    variants = {"ovr_decomp": lambda: OneVsRestSVC(device="cuda:0", solver="decomp"),
                "ovo_w10": lambda: OneVsOneSVC(device="cuda:0"),
                "ovo_w5": lambda: OneVsOneSVC(device="cuda:0", concurrent_solves=5),
                "ovo_w45": lambda: OneVsOneSVC(device="cuda:0", concurrent_solves=45)}
    res = {k: {"fit_s": []} for k in variants}
    for rep in range(reps + 1):  # rep 0: the warm-up of every variant (pool threads, contexts, slabs)
        for name, make in variants.items():
            m = make().fit(X, tr.labels)
            torch.cuda.synchronize()
            if rep:
                res[name]["fit_s"].append(m.fit_time_)
            if rep == reps:
                t0 = time.perf_counter()
                acc = m.score(Xt, te.labels)
                res[name].update(accuracy=acc, predict_s=time.perf_counter() - t0, n_sv_union=int(len(m.support_)),
                                 stop_reasons=sorted(set(m.stop_reasons_)), timings={k: v for k, v in m.timings_.items()})
                if name.startswith("ovo"):
                    per = [t["total_ms"] for t in m.pair_timings_.values()]
                    res[name]["pair_total_ms"] = {"min": min(per), "median": statistics.median(per), "max": max(per),
                                                  "sum": sum(per)}
                    res[name]["n_support"] = m.n_support_.tolist()
                    res[name]["pair_iterations"] = {"min": int(m.n_iter_.min()), "max": int(m.n_iter_.max())}
            print(name, "rep", rep, f"fit {m.fit_time_:.3f} s", flush=True)
    out["fit"] = res
    return OneVsOneSVC(device="cuda:0").fit(X, tr.labels)


def predict_part(model, te, kreps, out):
    dm = model._dev_model
    Xt = te.compact().X
    k, S, P = len(model.classes_), len(model.support_), len(model.rho_)
    Xq = D.upload_rows(Xt, dm["device"])
    _, _, nq = D.minmax_scale_(Xq, dm["d"], dm["mn"], dm["mx"])
    gamma = model.params.gamma
    Kq = D.rbf_gram(Xq, nq, dm["Xs"], dm["ns"], gamma)
    m, ldk = Kq.shape
    # the dense baseline: S x P coefficients (zero where a support vector's class is not in the pair), votes in torch
    start = np.concatenate([[0], np.cumsum(model.n_support_)])
    dense = np.zeros((S, P))
    first = np.zeros((P, k), dtype=np.float64)
    second = np.zeros((P, k), dtype=np.float64)
    for p, (a, b) in enumerate(model._pairs):
        dense[start[a]:start[a + 1], p] = model.dual_coef_[b - 1, start[a]:start[a + 1]]
        dense[start[b]:start[b + 1], p] = model.dual_coef_[a, start[b]:start[b + 1]]
        first[p, a] = second[p, b] = 1.0
    dense_d, first_d, second_d = (torch.from_numpy(x).to(Kq.device) for x in (dense, first, second))
    tie = torch.arange(k, 0, -1, device=Kq.device, dtype=torch.float64) / (2.0 * k)  # the lowest index wins a tie

    def baseline():
        dec = torch.matmul(Kq[:, :S], dense_d) - dm["rho"]
        win = (dec > 0).to(torch.float64)
        votes = win @ first_d + (1.0 - win) @ second_d
        return dec, torch.argmax(votes + tie, dim=1)

    def matmul_only():
        return torch.matmul(Kq[:, :S], dense_d)

    dec_k, lab_k = D.ovo_votes(Kq, dm["start"], dm["coef"], dm["rho"], nsv=S)
    dec_b, lab_b = baseline()
    r = {"m": m, "S": S, "k": k, "P": P, "ldk": ldk, "K_block_bytes": m * ldk * 8, "coef_bytes": (k - 1) * S * 8,
         "dense_zero_share": float((dense == 0).mean()),
         "max_abs_dec_diff_kernel_vs_baseline": float((dec_k - dec_b).abs().max()),
         "labels_differ": int((lab_k.to(torch.int64) != lab_b).sum())}
    r["cross_kernel"] = _events(lambda: D.rbf_gram(Xq, nq, dm["Xs"], dm["ns"], gamma, out=Kq), kreps)
    r["vote_kernel"] = _events(lambda: D.ovo_votes(Kq, dm["start"], dm["coef"], dm["rho"], nsv=S), kreps)
    r["vote_kernel_labels_only"] = _events(lambda: D.ovo_votes(Kq, dm["start"], dm["coef"], dm["rho"], want_dec=False,
                                                               nsv=S), kreps)
    r["baseline_matmul_and_vote"] = _events(baseline, kreps)
    r["baseline_matmul_only"] = _events(matmul_only, kreps)
    r["ovo_predict_device"] = _events(lambda: D.ovo_predict(dm["Xs"], dm["ns"], Xq, nq, gamma, dm["start"], dm["coef"],
                                                            dm["rho"]), kreps)
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        model.predict(Xt)
        t.append(time.perf_counter() - t0)
    r["predict_end_to_end_ms"] = {"median_ms": statistics.median(t) * 1e3, "min_ms": min(t) * 1e3}
    r["vote_kernel_K_bytes_per_s"] = r["K_block_bytes"] / (r["vote_kernel"]["median_ms"] * 1e-3)
    out["predict"] = r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--kreps", type=int, default=20)
    ap.add_argument("--part", choices=["fit", "predict", "all"], default="all")
    ap.add_argument("--out", default="ovo_profile.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ovo_profile.py measures on a GPU: none is visible")
    tr, te = synthetic_mnist(a.n, seed=a.seed), synthetic_mnist(a.m, seed=a.seed, offset=a.n)
    out = {"n": a.n, "m": a.m, "seed": a.seed, "device": torch.cuda.get_device_name(0)}
    model = None
    if a.part in ("fit", "all"):
        model = fit_part(tr, te, a.reps, out)
    if a.part in ("predict", "all"):
        if model is None:
            model = OneVsOneSVC(device="cuda:0").fit(tr.compact().X, tr.labels)
        predict_part(model, te, a.kreps, out)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
