"""Host-side filter design of spy.preprocessing, in float64: windowed-sinc kernels and their minimum-phase version
(the contract of syncopy/preproc/firws.py: design_wsinc, minphaserceps) and Butterworth second-order sections with
SciPy's start state and padding (scipy.signal.butter / sosfilt_zi / sosfiltfilt).  A few thousand numbers per call;
the samples themselves never pass through here."""
import numpy as np
import scipy.signal as sps
import scipy.signal.windows as spw

WINDOWS = ("hamming", "hann", "blackman")
FILTER_TYPES = ("lp", "hp", "bp", "bs")


def _lowpass(window, order, fc):
    """order + 1 taps (order even): sin(2 pi fc m) / m around the centre tap 2 pi fc, times the window, unit DC gain."""
    w = 2.0 * np.pi * fc
    m = np.arange(1, order / 2 + 1)
    side = np.sin(w * m) / m
    taps = np.hstack([side[::-1], w, side]) * getattr(spw, window)(order + 1)
    return taps / taps.sum()


def _spectral_inversion(taps):
    """delta - taps: the complementary high-pass of a low-pass with an odd number of taps"""
    out = -taps
    out[len(out) // 2] += 1.0
    return out


def windowed_sinc(window, order, fc, filter_type="lp"):
    """Windowed-sinc FIR kernel; `fc` in units of the sampling rate (a pair, low to high, for "bp" / "bs").  An odd
    order is raised by one; the kernel has order + 1 taps."""
    order = int(order) + int(order) % 2
    if filter_type == "lp":
        return _lowpass(window, order, fc)
    if filter_type == "hp":
        return _spectral_inversion(_lowpass(window, order, fc))
    lo, hi = fc
    if filter_type == "bs":           # what passes below `lo` plus what passes above `hi`
        return _lowpass(window, order, lo) + _spectral_inversion(_lowpass(window, order, hi))
    # band-pass: low-pass at `hi` plus high-pass at `lo` passes the band twice and everything else once - take the
    # all-pass (a unit centre tap) away again
    taps = _lowpass(window, order, hi) + _spectral_inversion(_lowpass(window, order, lo))
    taps[len(taps) // 2] -= 1.0
    return taps


def minimum_phase(taps):
    """Minimum-phase kernel with the magnitude response of `taps` through the real cepstrum: zero-padded about 1000-fold
    to a power of two, magnitudes clipped at 1e-8 (-160 dB), the cepstrum folded onto its causal half, exponentiated."""
    n = len(taps)
    nfft = int(2 ** np.ceil(np.log2(n * 1e3)))
    mag = np.abs(np.fft.fft(taps, nfft))
    mag[mag < 1e-8] = 1e-8
    ceps = np.real(np.fft.ifft(np.log(mag)))
    half = nfft // 2
    folded = np.zeros(nfft - 1)      # one sample short of nfft: the reference transforms back at this length, kept
    folded[0] = ceps[0]
    folded[1:half] = ceps[1:half] + ceps[nfft - 1:half:-1]       # c[k] + c[-k]
    folded[half] = ceps[half]
    return np.real(np.fft.ifft(np.exp(np.fft.fft(folded))))[:n]


def butterworth(order, freq, filter_type, samplerate):
    """(sos, zi, edge): second-order sections, sosfilt_zi and the odd-extension length sosfiltfilt uses for them
    (3 * ntaps with ntaps = 2 * n_sections + 1 less the zero-padded sections)."""
    sos = sps.butter(int(order), freq, filter_type, fs=samplerate, output="sos")
    zi = sps.sosfilt_zi(sos)
    ntaps = 2 * sos.shape[0] + 1
    ntaps -= min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))
    return np.ascontiguousarray(sos), np.ascontiguousarray(zi), 3 * ntaps
