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


def resample(x, taps_scaled, up, down):
    return resample64(x, taps_scaled, up, down).astype(np.float32)


def downsample(x, skip):
    return np.asarray(x)[::skip]


RESAMPLE_OPS = {"resample": resample, "downsample": downsample, "fir": PO.fir}
