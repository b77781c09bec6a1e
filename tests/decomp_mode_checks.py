"""What the device entries of the decomposition solver's modes refuse (csrc/include/decomp_mode.h), through
``svm355.ops.device``: shared by test_gpu_svr.py, test_gpu_oneclass.py and test_gpu_probability.py.  The cells are
the refused ones of tests/test_decomp_modes_cpu.py's matrix that a device entry can express."""
import numpy as np
import pytest
import torch

from svm355 import SVMParams
from svm355 import _native as N
from svm355.ops import device as D

# feature -> (the parameters that ask for it, its phrase)
FEATURES = {
    "shrinking": (dict(shrinking=True), "shrinking"),
    "newton": ({}, "the Newton polish (SVM355_DECOMP_NEWTON)"),
    "weights": (dict(weight_pos=2.0), "class weights"),
}


def pixel_rows(dev):
    """64 uint8 rows x 16 columns on the device (every column spans 0 .. 255: the exact-integer plan), their column
    bounds on the host, and +1 / -1 labels on the device."""
    X = np.random.default_rng(5).integers(0, 256, (64, 16), dtype=np.uint8)
    X[0], X[1] = 0, 255
    Xu = D.upload_u8(X, dev)
    mm = torch.empty(32, dtype=torch.float64, device=dev)
    D.minmax_u8(Xu, out=mm)
    mm = mm.cpu().numpy()
    y = torch.from_numpy(np.where(np.arange(64) % 2 == 0, 1, -1).astype(np.int32)).to(dev)
    return Xu, mm[:16].copy(), mm[16:].copy(), y


def check_refusal(entry, solve, feature, call, rows, monkeypatch):
    """``call(params)`` runs the mode's wrapper on ``rows``: it raises under the entry's name with the mode's and the
    feature's phrase, and -- the refusal comes before the context's stream is joined -- leaves the context usable:
    a plain solve of the same rows converges."""
    Xu, mn, mx, y = rows
    kw, phrase = FEATURES[feature]
    if feature == "newton":
        monkeypatch.setenv("SVM355_DECOMP_NEWTON", "1")
    with pytest.raises(N.NativeError) as ei:
        call(SVMParams(gamma=0.5, **kw))
    assert str(ei.value).startswith(entry)
    assert N.last_error() == f"{entry}: the {solve} solve does not support {phrase}"
    monkeypatch.delenv("SVM355_DECOMP_NEWTON", raising=False)
    alpha = torch.empty(64, dtype=torch.float64, device=Xu.device)
    out = D.train_decomp(Xu, y, alpha, SVMParams(gamma=0.5), mn, mx)
    assert out is not None and out[0].stop_reason == "converged"
