"""Float64 oracle of the Hilbert option of spy.preprocessing and the routine table that carries it: the analytic signal
scipy.signal.hilbert(trial.astype(float64), axis=0), circular over the trial length, followed by the reference's
spectralConversions[output] (shared/const_def.py:25-37), written from the contract."""
import numpy as np
import scipy.signal as sps

from preproc_oracle import PREPROC_OPS

OUTPUTS = ("abs", "complex", "real", "imag", "absreal", "absimag", "angle")

CONVERSIONS = {
    "abs": np.absolute,
    "complex": lambda z: z,
    "real": np.real,
    "imag": np.imag,
    "absreal": lambda z: np.absolute(np.real(z)),
    "absimag": lambda z: np.absolute(np.imag(z)),
    "angle": np.angle,
}


def analytic64(x):
    """complex128 analytic signal of a (time, channel) trial or a (trial, time, channel) batch along time"""
    x = np.asarray(x, dtype=np.float64)
    return sps.hilbert(x, axis=x.ndim - 2)


def hilbert64(x, output):
    """the oracle, unrounded: float64 (complex128 for "complex")"""
    return CONVERSIONS[output](analytic64(x))


def hilbert(x, output):
    """the routine of the model table: one float32 (time, channel) trial -> float32, or complex64 for "complex".  A
    channel that holds a non-finite sample comes back all-NaN (SciPy leaves a mix of inf and NaN there)."""
    x = np.asarray(x, dtype=np.float32)
    ok = np.isfinite(x).all(axis=0)
    z = np.full(x.shape, np.nan + 1j * np.nan, dtype=np.complex128)
    if ok.any():
        z[:, ok] = analytic64(x[:, ok])
    return CONVERSIONS[output](z).astype(np.complex64 if output == "complex" else np.float32)


def has_nan(x):
    """the trial flag once a Hilbert step closes the chain: the device kernels report non-finite samples"""
    return bool(not np.isfinite(x).all())


HILBERT_OPS = dict(PREPROC_OPS, hilbert=hilbert)
