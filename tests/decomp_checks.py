"""Checks shared by the decomposition solver's GPU tests (test_gpu_decomp.py, test_gpu_decomp_oracle.py)."""
import numpy as np
import torch


def kkt_gap_fp64(X, y, a, p):
    """b_low - b_high over ALL points from an independent FP64 RBF (torch, min-max scaled rows)."""
    dev = torch.device("cuda:0")
    Xs = torch.from_numpy(X.astype(np.float64)).to(dev)
    mn, mx = Xs.min(0).values, Xs.max(0).values
    rng = torch.where(mx - mn < 1e-12, torch.ones_like(mx), mx - mn)
    Xs = (Xs - mn) / rng
    sq = (Xs * Xs).sum(1)
    ay = torch.from_numpy(a * y).to(dev)
    f = torch.empty(len(y), dtype=torch.float64, device=dev)
    for i0 in range(0, len(y), 4096):
        B = Xs[i0:i0 + 4096] @ Xs.T
        Kb = torch.exp(-p.gamma * torch.clamp(sq[i0:i0 + 4096, None] + sq[None, :] - 2.0 * B, min=0.0))
        f[i0:i0 + 4096] = Kb @ ay
    f = f.cpu().numpy() - y
    hi = ((y == 1) & (a < p.C - p.eps)) | ((y == -1) & (a > p.eps))
    lo = ((y == 1) & (a > p.eps)) | ((y == -1) & (a < p.C - p.eps))
    return f[lo].max() - f[hi].min()
