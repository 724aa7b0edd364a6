"""Module-wide constants (values of syncopy/shared/const_def.py:12-62)."""
import numpy as np
from scipy.signal import windows

spectralDTypes = {
    "pow": np.float32, "abs": np.float32, "real": np.float32, "imag": np.float32, "angle": np.float32,
    "absreal": np.float32, "absimag": np.float32, "fourier": np.complex64, "complex": np.complex64,
}

availableTapers = [w for w in windows.__all__ if w not in ("get_window", "exponential", "dpss")]
availablePaddingOpt = ["maxperlen", "nextpow2"]
availableMethods = ("mtmfft", "mtmconvol", "wavelet", "superlet", "welch")
connectivityMethods = ("coh", "corr", "csd", "granger", "ppc", "plv", "pli", "wpli", "wpli_debiased", "dtf", "pdc",
                       "amplcorr", "powcorr", "powcorr_ortho", "psi")
# ppc and its siblings beyond the reference: non-linear in the single-trial cross spectrum, accumulated over trials
phaseMethods = ("ppc", "plv", "pli", "wpli", "wpli_debiased")
# beyond the reference as well: directed measures of the Wilson factors, which take every rule of granger
directedMethods = ("dtf", "pdc")
# and the envelope correlations (Hipp et al. 2012): correlations over the repetitions (trial x taper) of quantities that
# are non-linear in the spectra; they behave as ppc does, on the batched route only
envelopeMethods = ("amplcorr", "powcorr", "powcorr_ortho")
connectivity_outputs = {"abs", "pow", "complex", "fourier", "angle", "real", "imag"}
