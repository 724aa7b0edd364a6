"""The float64 wavelet path (cwt64_kernel.h) against the oracle: the reference computation and the criterion shared by the
emulator and GPU tests (TEST INFRASTRUCTURE ONLY)."""
import numpy as np

from oracle import spy_oracle as O

# Both sides of the float64 comparisons are float64 FFT convolutions of the same float32 (detrended) input, rounded to
# complex64 where the reference stores its result: they may differ by the rounding of that one step.  A complex64
# coefficient, its real and its imaginary part: one float32 rounding, |d| <= 2^-23 |ref|.  pow and abs are computed from
# the rounded coefficient in float32 (x^2 + y^2, hypot): a coefficient off by one rounding moves them by ~2 ulp, the
# float32 arithmetic on top by ~1 more (measured: 1.0 / 1.34 ulp at most) - four ulp.  The absolute term covers the
# float64 convolutions' own error where a coefficient is tiny next to the trial's largest.
CWT64_ULPS = {"fourier": 1, "real": 1, "imag": 1, "pow": 4, "abs": 4}


def cwt64_taps(nsig, scales, dt, w0=6.0, family=None, order=None, sl_cycles=None):
    """The sampled kernels of spyhip_cwt_plan_create trimmed to the taps that can overlap a signal of nsig samples, and
    each trimmed kernel's "same" offset: [(taps, centre)].  family None / "Paul" / "DOG" as O.cwt_kernel; `sl_cycles`:
    MorletSL (O.cwt_sl)."""
    out = []
    for s in scales:
        if sl_cycles is None:
            h = O.cwt_kernel(s, dt, w0, family, order)
        else:
            M = 10 * s * sl_cycles / dt
            t = np.arange((-M + 1) / 2.0, (M + 1) / 2.0) * dt
            h = dt ** 0.5 / (4 * np.pi) * O.morlet_sl(t, s, sl_cycles)
        h = np.asarray(h, dtype=np.complex128)
        c = (h.size - 1) // 2
        m0, m1 = max(0, c - (nsig - 1)), min(h.size, c + nsig)
        out.append((h[m0:m1], c - m0))
    return out


def cwt64_ref(data, ss, lo, hi, nsig, scales, detrend, output, chan_idx=None, family=None, order=None, sl_cycles=None,
              convert=True):
    """Per segment: O.cwt of the float32-detrended trial in float64 (complex64 storage) -> (nseg, nsig, nscales, nchan)."""
    cols = np.arange(data.shape[1]) if chan_idx is None else np.asarray(chan_idx)
    res = []
    for s, a, b in zip(ss, lo, hi):
        trial = O.detrend(np.ascontiguousarray(data[a:b][:, cols]), None if detrend < 0 else detrend)   # C order, as a trial is
        x = trial[s - a:s - a + nsig].astype(np.float64)
        if sl_cycles is None:
            y = O.cwt(x, 1000.0, scales, 6.0, family, order)
        else:
            y = O.cwt_sl(x, sl_cycles, scales, 1e-3)
        y = y.transpose(1, 0, 2)
        res.append(O.convert_output(y, output) if convert else y)
    return np.stack(res)


def assert_cwt64(got, ref, output, what, nterms=1, scale=None, amax=None):
    """|got - ref| <= ulps * 2^-23 * scale + 1e-12 * amax elementwise (scale = |ref|; sums of `nterms` rounded terms:
    their sum of moduli times nterms; amax = max|ref|, or the largest coefficient modulus of the transform where the
    output alone does not show it - the imaginary part of a real (DOG) kernel's transform is float64 noise about 0)."""
    g = np.asarray(got).astype(np.complex128)
    r = np.asarray(ref).astype(np.complex128)
    assert g.shape == r.shape, (g.shape, r.shape)
    sc = np.abs(r) if scale is None else scale
    bound = CWT64_ULPS[output] * nterms * 2.0 ** -23 * sc + 1e-12 * (np.abs(r).max() if amax is None else amax)
    err = np.abs(g - r)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements beyond float32 rounding; worst at {i}: "
                             f"got {g[i]} ref {r[i]} (bound {bound[i]:.3g})")
