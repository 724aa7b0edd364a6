"""NumPy / SciPy model of the steps of spy.resampledata (syncopy preproc/resampling.py: resample, downsample), written
from the contract, in the `routine_classes` shape that syncopy_amd.preproc.resampledata takes with
compute_method="sequential": every function maps one (time, channel) float32 trial to the next stage's trial."""
import numpy as np
import scipy.signal as sps

import preproc_oracle as PO


def resample64(x, taps_scaled, up, down):
    """scipy.signal.resample_poly in float64 with the caller's taps (it multiplies them by `up` itself: undone here)"""
    taps = np.asarray(taps_scaled, dtype=np.float64) / up
    return sps.resample_poly(np.asarray(x, dtype=np.float64), up, down, window=taps, axis=0)


def upfirdn64(x, taps, up, down):
    """resample64 without resample_poly's first step, the division of up and down by their common factor (3 / 18 is
    filtered as 1 / 6 there, with the taps taken at the lower rate: another operation).  The kernel takes the pair as it is
    given; this is resample_poly's own padding, scipy.signal.upfirdn call and cut.  Equal to resample64 on a reduced pair."""
    x, taps = np.asarray(x, dtype=np.float64), np.asarray(taps, dtype=np.float64)
    nout = -(-x.shape[0] * up // down)
    half = (len(taps) - 1) // 2
    pre = down - half % down
    skip = (half + pre) // down
    post = 0
    while -(-((x.shape[0] - 1) * up + len(taps) + pre + post) // down) < nout + skip:
        post += 1
    h = np.concatenate([np.zeros(pre), taps, np.zeros(post)])
    return sps.upfirdn(h, x, up, down, axis=0)[skip:skip + nout]


def resample(x, taps_scaled, up, down):
    return resample64(x, taps_scaled, up, down).astype(np.float32)


def downsample(x, skip):
    return np.asarray(x)[::skip]


RESAMPLE_OPS = {"resample": resample, "downsample": downsample, "fir": PO.fir}
