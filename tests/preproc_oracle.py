"""NumPy / SciPy model of the steps of spy.preprocessing (syncopy preproc/compRoutines.py and preproc/firws.py), written
from the contract, in the `routine_classes` shape that syncopy_amd.preproc.preprocessing takes with
compute_method="sequential": every function maps one (time, channel) float32 trial to the next stage's trial."""
import numpy as np
import scipy.signal as sps


def detrend(x, order):
    """order 0: SciPy / NumPy on the float32 array itself (the summation order is part of the contract); order 1: the
    least-squares line in float64.  A channel with a NaN comes back all-NaN."""
    x = np.asarray(x, dtype=np.float32)
    if order == 0:
        return sps.detrend(x, type="constant", axis=0)
    out = np.full(x.shape, np.nan, dtype=np.float64)
    ok = ~np.isnan(x).any(axis=0)
    if ok.any():
        out[:, ok] = sps.detrend(x[:, ok].astype(np.float64), type="linear", axis=0)
    return out.astype(np.float32)


def standardize(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x - np.mean(x, axis=0)) / np.std(x, axis=0)


def sosfilt(x, sos):
    return sps.sosfilt(sos, np.asarray(x, dtype=np.float32), axis=0).astype(np.float32)


def sosfiltfilt(x, sos, zi=None, edge=None):
    return sps.sosfiltfilt(sos, np.asarray(x, dtype=np.float32), axis=0).astype(np.float32)


def fir64(x, taps):
    """mode="same" convolution as a direct float64 sum, per channel (float64 result)"""
    x = np.asarray(x, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    start = (len(taps) - 1) // 2
    out = np.empty(x.shape, dtype=np.float64)
    for c in range(x.shape[1]):
        out[:, c] = np.convolve(x[:, c], taps, mode="full")[start:start + x.shape[0]]
    return out


def fir(x, taps):
    return fir64(x, taps).astype(np.float32)


def has_nan(x):
    return bool(np.isnan(x).any())


def rectify(x):
    return np.abs(x)


PREPROC_OPS = {"detrend": detrend, "standardize": standardize, "sosfilt": sosfilt, "sosfiltfilt": sosfiltfilt, "fir": fir,
               "has_nan": has_nan, "rectify": rectify}
